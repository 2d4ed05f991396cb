"""The hybrid render (chroma/cuda/hybrid_render.cu, chroma/camera.py:188-249) on the GPU.

Every sample of the lookup and image passes is rebuilt on the host: the draws from oracle.uniform_stream, the first hit from
oracle.distance_to_mesh, the polarisation from oracle.math_fn('sin' / 'cos'), then oracle.propagate stepped one step at a time
until the first diffuse reflection.  The diffusing triangle, its side, the history and the final draw counter must equal the
kernel's sample outputs.  Tables, image and pixels must equal their NumPy restatements (chroma_amd.gpu.render) bit for bit.

The comparands here are the project's own restatements of hybrid_render.cu.  What holds THEM to the reference is
tests/test_ref_hybrid_host.py (oracle_lookup, oracle_image, oracle.to_diffuse, hybrid_accumulate, hybrid_image_update and
hybrid_pixels against the reference's own file compiled for the host, libm and contract builds; hence the `variant` keyword of
the helpers below), and tests/test_gpu_ref_hybrid.py compares the kernels with that build directly."""
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

from chroma_amd.event import NAN_ABORT, REFLECT_DIFFUSE, TERMINAL_MASK
from conftest import ROOT, make_box_geometry

pytestmark = pytest.mark.gpu

f32 = np.float32


# The demo detectors have no diffusing surface (a black outer sphere, black world box): the scenes here give them a grey one.
GREY_SCENES = """
from chroma_amd.geometry import Surface


def _grey():
    grey = Surface('grey')
    grey.set('reflect_diffuse', 0.6)
    grey.set('reflect_specular', 0.1)
    grey.set('absorb', 0.3)
    return grey


def grey_tiny():
    import chroma_amd.demo as demo
    black = demo.black_surface
    demo.black_surface = _grey()                 # the outer sphere, behind the PMTs and their shiny cones
    try:
        return demo.tiny()
    finally:
        demo.black_surface = black


def grey_stress():
    from chroma_amd.demo.stress import scintillator_stress
    from chroma_amd.geometry import Solid, vacuum
    from chroma_amd.make import box
    det = scintillator_stress()
    det.add_solid(Solid(box(1800.0, 1800.0, 1800.0), vacuum, vacuum, surface=_grey()))     # walls around the scintillator cube
    return det
"""


def _scene(name):
    from chroma_amd.loader import create_geometry_from_obj
    ns = {}
    exec(compile(GREY_SCENES, 'grey_scenes', 'exec'), ns)
    return create_geometry_from_obj(ns[name]())


# ---- host restatements ------------------------------------------------------------------------------------------
def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _normalize(a):
    return a / np.sqrt(_dot(a, a))[:, None]


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def _vertices(geometry):
    v = np.asarray(geometry.mesh.vertices, f32)
    t = np.asarray(geometry.mesh.triangles, np.int64)
    return v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]


def _normals(geometry):
    v0, v1, v2 = _vertices(geometry)
    return _normalize(_cross(v1 - v0, v2 - v1))


def _uniform_sphere(oracle_mod, u_theta, u_z, variant='contract'):
    """random.h:15-23 with the contract's sin / cos (uniform_sphere of propagate_device.h)."""
    theta = f32(0) + u_theta * (f32(2 * f32(np.pi)) - f32(0))
    u = f32(-1) + u_z * (f32(1) - f32(-1))
    c = np.sqrt(f32(1) - u * u)
    return np.stack([c * oracle_mod.math_fn('cos', theta, variant=variant), c * oracle_mod.math_fn('sin', theta, variant=variant), u],
                    axis=1).astype(f32)


def _draws(oracle_mod, seed, id_base, counters, n):
    return np.array([oracle_mod.uniform_stream(seed, id_base + k, n, start=int(counters[k])) for k in range(len(counters))],
                    f32).reshape(len(counters), n)


def _step_to_diffuse(oracle_mod, packed, normals, photons, active, seed, id_base, counters, max_steps):
    """oracle.propagate stepped one step at a time, each sample stopped at its first diffuse reflection (or when it ends).
    Returns (triangle or -1, side, history, counters)."""
    from chroma_amd.event import Photons
    n = len(photons)
    cur = [np.array(a, copy=True) for a in (photons.pos, photons.dir, photons.pol, photons.wavelengths, photons.t,
                                             photons.last_hit_triangles, photons.flags, photons.weights, photons.evidx)]
    ctr = np.array(counters, np.uint32, copy=True)
    done = ~np.asarray(active, bool)
    side = np.zeros(n, np.uint32)
    for _ in range(max_steps):
        if done.all():
            break
        flags_in = cur[6].copy()
        flags_in[done] |= np.uint32(NAN_ABORT)                    # frozen: the oracle leaves terminal photons untouched
        out, ctr_new, _ = oracle_mod.propagate(packed, Photons(*(cur[:6] + [flags_in] + cur[7:])), seed, photon_id_base=id_base,
                                               max_steps=1, rng_counters=ctr)
        outs = [out.pos, out.dir, out.pol, out.wavelengths, out.t, out.last_hit_triangles, out.flags, out.weights, out.evidx]
        stepping = ~done
        lh = np.asarray(out.last_hit_triangles)
        hit = stepping & (lh >= 0)
        d_in = np.asarray(cur[1], f32).reshape(-1, 3)[hit]
        side[hit] = (~(_dot(normals[lh[hit]], -d_in) > f32(0))).astype(np.uint32)
        for a, b in zip(cur, outs):
            a[stepping] = np.asarray(b)[stepping]
        ctr[stepping] = ctr_new[stepping]
        fl = np.asarray(out.flags)
        done |= stepping & (((fl & REFLECT_DIFFUSE) != 0) | ((fl & TERMINAL_MASK) != 0))
    diffuse = np.asarray(active, bool) & ((cur[6] & REFLECT_DIFFUSE) != 0)
    tri = np.where(diffuse, cur[5], -1).astype(np.int32)
    return tri, np.where(diffuse, side, 0).astype(np.uint32), np.where(active, cur[6], 0).astype(np.uint32), ctr


def _to_diffuse(oracle_mod, packed, photons, active, seed, id_base, counters, max_steps, variant='contract'):
    """oracle.to_diffuse: the reference's own loop (hybrid_render.cu:20-58), which takes direction and polarisation as the
    kernel made them.  _step_to_diffuse goes through oracle.propagate, which divides both by their norms at every step as
    propagate.cu does on load: the same samples, but for a ray that grazes a triangle (where an ulp of the direction decides
    what it meets next).  Returns (triangle or -1, side, history, counters) like _step_to_diffuse."""
    active = np.asarray(active, bool)
    out, ctr, side = oracle_mod.to_diffuse(packed, photons, seed, photon_id_base=id_base, max_steps=max_steps, rng_counters=counters,
                                           active=active, variant=variant)
    flags = np.asarray(out.flags, np.uint32)
    diffuse = active & ((flags & REFLECT_DIFFUSE) != 0)
    tri = np.where(diffuse, out.last_hit_triangles, -1).astype(np.int32)
    return tri, np.where(diffuse, side, 0).astype(np.uint32), np.where(active, flags, 0).astype(np.uint32), ctr


def oracle_lookup(oracle_mod, packed, geometry, seed, id_base, counters, nthreads, offset, source, wavelength, max_steps,
                  variant='contract'):
    """One update_xyz_lookup launch restated.  Returns (triangle, side, history, cos_theta, counters) of its samples."""
    from chroma_amd.event import Photons
    ntri = len(geometry.mesh.triangles)
    n = max(0, min(offset + nthreads, ntri) - offset)
    c0 = np.asarray(counters, np.uint32)[:n]
    u = _draws(oracle_mod, seed, id_base, c0, 4)
    v0, v1, v2 = [x[offset:offset + n] for x in _vertices(geometry)]
    a = u[:, 0]
    b = f32(0) + u[:, 1] * ((f32(1) - a) - f32(0))
    c = (f32(1) - a) - b
    pos = np.tile(np.asarray(source, f32), (n, 1))
    d = ((a[:, None] * v0 + b[:, None] * v1) + c[:, None] * v2) - pos
    d = d / np.sqrt(_dot(d, d))[:, None]
    # update_xyz_lookup casts the direction it has normalised itself (hybrid_render.cu:84-87); distance_to_mesh would divide
    # it by its norm once more and move a grazing ray by an ulp onto another triangle
    _, first, _ = oracle_mod.distance_to_mesh(packed, pos, d, normalize=False, variant=variant)
    mine = first == np.arange(offset, offset + n)
    nrm = _normals(geometry)[offset:offset + n]
    cos = _dot(nrm, -d)
    cos = np.where(cos < f32(0), _dot(-nrm, -d), cos).astype(f32)
    cos[~mine] = 0
    pol = _uniform_sphere(oracle_mod, u[:, 2], u[:, 3], variant=variant)
    photons = Photons(pos, d, pol, np.full(n, wavelength, f32), np.zeros(n, f32), np.full(n, -1, np.int32),
                      np.zeros(n, np.uint32), np.ones(n, f32), np.zeros(n, np.uint32))
    start = np.where(mine, c0 + 4, c0 + 2).astype(np.uint32)
    # (the keyword only where it says something: a test swaps _to_diffuse for a route of the contract build that takes none)
    tri, side, hist, ctr = _to_diffuse(oracle_mod, packed, photons, mine, seed, id_base, start, max_steps,
                                       **({} if variant == 'contract' else {'variant': variant}))
    return tri, side, hist, cos, ctr, mine


def oracle_image(oracle_mod, packed, geometry, seed, id_base, counters, origins, directions, wavelength, max_steps, variant='contract'):
    from chroma_amd.event import Photons
    n = len(origins)
    c0 = np.asarray(counters, np.uint32)[:n]
    u = _draws(oracle_mod, seed, id_base, c0, 2)
    pol = _uniform_sphere(oracle_mod, u[:, 0], u[:, 1], variant=variant)
    d = np.asarray(directions, f32).reshape(-1, 3)
    with np.errstate(invalid='ignore', divide='ignore'):            # a zero or NaN direction gives NaN, as on the device
        d = d / np.sqrt(_dot(d, d))[:, None]                        # update_xyz_image's direction /= norm(direction), in f32
    photons = Photons(np.asarray(origins, f32), d, pol, np.full(n, wavelength, f32), np.zeros(n, f32),
                      np.full(n, -1, np.int32), np.zeros(n, np.uint32), np.ones(n, f32), np.zeros(n, np.uint32))
    tri, side, hist, ctr = _to_diffuse(oracle_mod, packed, photons, np.ones(n, bool), seed, id_base, c0 + 2, max_steps,
                                       **({} if variant == 'contract' else {'variant': variant}))
    return tri, side, hist, ctr


# ---- device helpers -------------------------------------------------------------------------------------------------
def _renderer(geometry, size, source_inside=None, seed=7, max_steps=10):
    from chroma_amd import gpu
    from chroma_amd.render_cli import camera_rays
    from chroma_amd.tools import from_film
    gpu.create_cuda_context(0)
    if source_inside is None:
        point, pos, dirs = camera_rays(geometry, size)
    else:
        point = np.asarray(source_inside, float)
        pos, dirs = from_film(position=(0.0, 0.0, 0.0), axis1=(0, 0, 1), axis2=(1, 0, 0), size=size, width=35.0, focal_length=18.0)
    rays = gpu.GPURays(pos, dirs, max_alpha_depth=1)
    return gpu.GPUHybridRender(gpu.GPUGeometry(geometry), rays, seed=seed, max_steps=max_steps), point


def _samples(r, n, with_cos=True):
    from chroma_amd.gpu.tools import zeros
    out = [zeros(n, np.int32, r.ctx), zeros(n, np.uint32, r.ctx), zeros(n, np.uint32, r.ctx)]
    return out + [zeros(n, np.float32, r.ctx)] if with_cos else out


def _tables(r):
    return (r.xyz_lookup1_gpu.get().view(f32).reshape(-1, 3).copy(), r.xyz_lookup2_gpu.get().view(f32).reshape(-1, 3).copy())


def _bits(a):
    return np.asarray(a, f32).view(np.uint32)


def _check_lookup_pass(oracle_mod, r, packed, geometry, offset, source, wavelength, xyz):
    """One lookup launch: samples against the oracle, the tables' change against hybrid_accumulate."""
    from chroma_amd.gpu.render import hybrid_accumulate
    n = r.npixels
    l1, l2 = _tables(r)
    c0 = r.rng_counters.get()
    s = _samples(r, n)
    r.lookup_pass(n, r.ntriangles, offset, source, wavelength, xyz, samples=s)
    tri, side, hist, cos = [a.get() for a in s]
    m = max(0, min(n, r.ntriangles - offset))
    want = oracle_lookup(oracle_mod, packed, geometry, r.seed, 0, c0, n, offset, source, wavelength, r.max_steps)
    for name, got, w in (('triangle', tri[:m], want[0]), ('side', side[:m], want[1]), ('history', hist[:m], want[2])):
        assert np.array_equal(got, w), '%s differs for %d of %d samples' % (name, (got != w).sum(), m)
    assert np.array_equal(_bits(cos[:m]), _bits(want[3])), 'cos_theta'
    c1 = r.rng_counters.get()
    assert np.array_equal(c1[:m], want[4]), 'draw counters'
    assert np.array_equal(c1[m:], c0[m:]), 'threads past the last triangle draw nothing'
    contrib = (cos[:m, None] * np.asarray(xyz, f32)[None, :]).astype(f32)
    w1, w2 = hybrid_accumulate(l1, l2, tri[:m], side[:m], contrib)
    g1, g2 = _tables(r)
    assert np.array_equal(_bits(g1), _bits(w1)) and np.array_equal(_bits(g2), _bits(w2)), 'lookup tables'
    return tri[:m], want[5], c0, c1


def _check_image_pass(oracle_mod, r, packed, geometry, wavelength, xyz):
    from chroma_amd.gpu.render import hybrid_image_update
    n = r.npixels
    c0 = r.rng_counters.get()
    img0 = r.image_gpu.get().view(f32).reshape(-1, 3).copy()
    s = _samples(r, n, with_cos=False)
    r.image_pass(wavelength, xyz, samples=s)
    tri, side, hist = [a.get() for a in s]
    o = r.rays.pos.get().view(f32).reshape(-1, 3)
    d = r.rays.dir.get().view(f32).reshape(-1, 3)
    want = oracle_image(oracle_mod, packed, geometry, r.seed, 0, c0, o, d, wavelength, r.max_steps)
    for name, got, w in (('triangle', tri, want[0]), ('side', side, want[1]), ('history', hist, want[2])):
        assert np.array_equal(got, w), 'image %s differs for %d of %d rays' % (name, (got != w).sum(), n)
    assert np.array_equal(r.rng_counters.get(), want[3]), 'image draw counters'
    l1, l2 = _tables(r)
    img = hybrid_image_update(img0, tri, side, l1, l2, xyz, r.nlookup_calls)
    assert np.array_equal(_bits(r.image_gpu.get().view(f32).reshape(-1, 3)), _bits(img)), 'image'
    return tri


# ---- tests -------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
def test_contract_trig_is_the_device_sincos(oracle_mod):
    """The polarisation restatement's math_fn('sin' / 'cos') gives what the device's cm_sincosf gives: the device bomb
    (uniform_sphere twice per photon) equals its NumPy restatement."""
    from chroma_amd import gpu
    gpu.create_cuda_context(0)
    n = 4096
    photons = gpu.generate_bomb(n, seed=11, pos=(0, 0, 0)).get()
    u = np.array([oracle_mod.uniform_stream(11, 0xB0B0000000000000 + k, 4) for k in range(n)], f32)
    d = _uniform_sphere(oracle_mod, u[:, 0], u[:, 1])
    assert np.array_equal(_bits(np.asarray(photons.dir, f32).reshape(-1, 3)), _bits(d))


@pytest.mark.timeout(1200)
@pytest.mark.parametrize('which', ['tiny', 'stress'])
def test_samples_tables_and_image_match_the_oracle(oracle_mod, which):
    """Source and camera inside: photons cross PMT glass (Fresnel), shiny cones and photocathodes (tiny), or the
    scintillator's thin-film, WLS, dichroic and detecting faces (stress), before they diffuse on the grey walls."""
    from chroma_amd.gpu.geometry import pack_geometry
    from chroma_amd.gpu.render import HYBRID_COLORS, hybrid_pixels
    geometry = _scene('grey_' + which)
    size, reps = ((48, 32), 1) if which == 'tiny' else ((40, 30), 8)
    packed = pack_geometry(geometry)
    r, source = _renderer(geometry, size, source_inside=(37.0, -210.0, 55.0) if which == 'tiny' else (37.0, -410.0, 55.0))
    n = r.npixels
    offsets = sorted(set([0, n * (r.ntriangles // (2 * n)), n * (r.ntriangles // n)])) if r.ntriangles > n else [0]
    ndiffuse = nmine = 0
    for _ in range(reps):
        for wavelength, xyz in HYBRID_COLORS:
            for offset in offsets:
                tri, mine, _, _ = _check_lookup_pass(oracle_mod, r, packed, geometry, offset, source, wavelength, xyz)
                ndiffuse += (tri >= 0).sum()
                nmine += mine.sum()
    assert nmine > 0 and ndiffuse > 0, (nmine, ndiffuse)
    assert ndiffuse < nmine                          # some were absorbed, detected or lost on the way
    r.nlookup_calls = reps
    nimg = 0
    for wavelength, xyz in HYBRID_COLORS:
        nimg += (_check_image_pass(oracle_mod, r, packed, geometry, wavelength, xyz) >= 0).sum()
    assert nimg > 0
    r.nimages = 1
    r.process_image()
    px = r.pixels_gpu.get()
    assert np.array_equal(px, hybrid_pixels(r.image_gpu.get().view(f32), 1))
    assert (px != 0xFF000000).any()


@pytest.mark.timeout(600)
def test_lambertian_room(oracle_mod):
    """Inside a box of Lambertian walls with no bulk attenuation, every sample that reaches its own triangle diffuses there
    at the first step; the tables are the reduction of the NumPy-restated cos_theta values."""
    from chroma_amd.demo.optics import lambertian_surface
    from chroma_amd.geometry import Material
    from chroma_amd.gpu.geometry import pack_geometry
    from chroma_amd.gpu.render import hybrid_accumulate
    clear = Material('clear')
    clear.set('refractive_index', 1.0)
    clear.set('absorption_length', 1e30)
    clear.set('scattering_length', 1e30)
    geometry = make_box_geometry(size=1000.0, material=clear, surface=lambertian_surface)
    packed = pack_geometry(geometry)
    source = (37.0, -210.0, 55.0)
    r, _ = _renderer(geometry, (16, 8), source_inside=source)
    ntri = r.ntriangles
    want1, want2 = np.zeros((ntri, 3), f32), np.zeros((ntri, 3), f32)
    nrm = _normals(geometry)
    v0, v1, v2 = _vertices(geometry)
    for rep in range(40):
        for wavelength, xyz in ((685.0, (1, 0, 0)), (445.0, (0, 0, 1))):
            c0 = r.rng_counters.get()
            s = _samples(r, r.npixels)
            r.lookup_pass(r.npixels, ntri, 0, source, wavelength, xyz, samples=s)
            tri, side, hist, cos = [a.get() for a in s]
            u = _draws(oracle_mod, r.seed, 0, c0[:ntri], 2)
            a = u[:, 0]
            b = f32(0) + u[:, 1] * ((f32(1) - a) - f32(0))
            c = (f32(1) - a) - b
            pos = np.tile(np.asarray(source, f32), (ntri, 1))
            d = ((a[:, None] * v0 + b[:, None] * v1) + c[:, None] * v2) - pos
            d = d / np.sqrt(_dot(d, d))[:, None]
            _, first, _ = oracle_mod.distance_to_mesh(packed, pos, d, normalize=False)
            mine = first == np.arange(ntri)
            assert mine.any()
            assert np.array_equal(tri[:ntri][mine], np.arange(ntri)[mine]) and (tri[:ntri][~mine] == -1).all()
            assert (hist[:ntri][mine] == REFLECT_DIFFUSE).all()
            ct = _dot(nrm, -d)
            ct = np.where(ct < f32(0), _dot(-nrm, -d), ct).astype(f32)
            assert np.array_equal(_bits(cos[:ntri][mine]), _bits(ct[mine]))
            sd = (~(_dot(nrm, -d) > f32(0))).astype(np.uint32)
            assert np.array_equal(side[:ntri][mine], sd[mine])
            contrib = (ct[:, None] * np.asarray(xyz, f32)[None, :]).astype(f32)
            hybrid_accumulate(want1, want2, np.where(mine, np.arange(ntri), -1), sd, contrib)
    g1, g2 = _tables(r)
    assert np.array_equal(_bits(g1), _bits(want1)) and np.array_equal(_bits(g2), _bits(want2))
    assert (g1 != 0).any() or (g2 != 0).any()


@pytest.mark.timeout(600)
def test_second_call_continues_the_streams(oracle_mod):
    from conftest import make_stress_geometry
    from chroma_amd.gpu.geometry import pack_geometry
    geometry = make_stress_geometry()
    packed = pack_geometry(geometry)
    r, source = _renderer(geometry, (8, 8), source_inside=(37.0, -210.0, 55.0))
    tri1, _, c0, c1 = _check_lookup_pass(oracle_mod, r, packed, geometry, 0, source, 545.0, (0, 1, 0))
    tri2, _, c1b, c2 = _check_lookup_pass(oracle_mod, r, packed, geometry, 0, source, 545.0, (0, 1, 0))
    m = len(tri1)
    assert np.array_equal(c1, c1b) and (c2[:m] > c1[:m]).all() and (c1[:m] > c0[:m]).all()
    u1 = _draws(oracle_mod, r.seed, 0, c0[:m], 1)
    u2 = _draws(oracle_mod, r.seed, 0, c1[:m], 1)
    assert not np.array_equal(u1, u2)


def _run_twice(geometry, size, seed):
    out = []
    for _ in range(2):
        r, source = _renderer(geometry, size, seed=seed)
        pixels = r.snapshot(source, nlookup=1, nimages=1)
        out.append((_tables(r), r.image_gpu.get().view(f32).copy(), pixels, r.rng_counters.get()))
    return out


@pytest.mark.timeout(900)
def test_reference_shaped_calls_and_determinism():
    """The camera's call sequence (camera.py:187-249) through get_cu_module('hybrid_render.cu') gives exactly what
    GPUHybridRender gives; two identical runs give identical bits."""
    from chroma_amd import gpu
    from chroma_amd.gpu.funcs import get_cu_module, GPUFuncs
    from chroma_amd.gpu.render import hybrid_pixels
    from chroma_amd.render_cli import camera_rays
    size, seed = (160, 120), 5
    tiny_geometry = _scene('grey_tiny')
    (a, b) = _run_twice(tiny_geometry, size, seed)
    for x, y in zip(a[0], b[0]):
        assert np.array_equal(_bits(x), _bits(y))
    assert np.array_equal(_bits(a[1]), _bits(b[1])) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    assert np.array_equal(a[2], hybrid_pixels(a[1], 1))
    assert (a[2] != 0xFF000000).sum() > 0.01 * len(a[2])                      # lit pixels (a single dim pass)

    ctx = gpu.create_cuda_context(0)
    gg = gpu.GPUGeometry(tiny_geometry)
    point, pos, dirs = camera_rays(tiny_geometry, size)
    rays = gpu.GPURays(pos, dirs)
    npixels = rays.pos.size
    funcs = GPUFuncs(get_cu_module('hybrid_render.cu', options=('--use_fast_math',)))
    rng_states = gpu.get_rng_states(npixels, seed=seed)
    ntri = len(tiny_geometry.mesh.triangles)
    l1 = gpu.zeros(ntri, gpu.vec.float3)
    l2 = gpu.zeros(ntri, gpu.vec.float3)
    image = gpu.zeros(npixels, gpu.vec.float3)
    pixels = gpu.empty(npixels, np.uint32)
    max_steps = 10
    for wavelength, rgb in zip([685.0, 545.0, 445.0], [(1, 0, 0), (0, 1, 0), (0, 0, 1)]):
        for i in range(l1.size // npixels + 1):
            funcs.update_xyz_lookup(np.int32(npixels), np.int32(l1.size), np.int32(i * npixels), gpu.vec.make_float3(*point),
                                    rng_states, np.float32(wavelength), gpu.vec.make_float3(*rgb), l1, l2, np.int32(max_steps),
                                    gg.gpudata, block=(64, 1, 1), grid=(npixels // 64 + 1, 1))
    nlookup_calls = 1
    for wavelength, rgb in zip([685.0, 545.0, 445.0], [(1, 0, 0), (0, 1, 0), (0, 0, 1)]):
        funcs.update_xyz_image(np.int32(rays.pos.size), rng_states, rays.pos, rays.dir, np.float32(wavelength),
                               gpu.vec.make_float3(*rgb), l1, l2, image, np.int32(nlookup_calls), np.int32(max_steps), gg.gpudata,
                               block=(64, 1, 1), grid=(rays.pos.size // 64 + 1, 1))
    funcs.process_image(np.int32(pixels.size), image, pixels, np.int32(1), block=(64, 1, 1), grid=(pixels.size // 64 + 1, 1))
    ctx.synchronize()
    assert np.array_equal(_bits(l1.get().view(f32).reshape(-1, 3)), _bits(a[0][0]))
    assert np.array_equal(_bits(l2.get().view(f32).reshape(-1, 3)), _bits(a[0][1]))
    assert np.array_equal(_bits(image.get().view(f32)), _bits(a[1]))
    assert np.array_equal(pixels.get(), a[2])


def _png_pixels(data):
    """(width, height, RGB rows) of an 8-bit RGB PNG with filter 0 on every row."""
    import struct
    assert data[:8] == b'\x89PNG\r\n\x1a\n'
    pos, idat, w, h = 8, b'', None, None
    while pos < len(data):
        (length,), kind = struct.unpack('>I', data[pos:pos + 4]), data[pos + 4:pos + 8]
        body = data[pos + 8:pos + 8 + length]
        if kind == b'IHDR':
            w, h = struct.unpack('>II', body[:8])
        elif kind == b'IDAT':
            idat += body
        pos += 12 + length
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + 3 * w)
    assert (raw[:, 0] == 0).all()
    return w, h, raw[:, 1:].reshape(h, w, 3)


@pytest.mark.timeout(900)
def test_cli_writes_the_snapshot(tmp_path):
    size, seed = (64, 48), 3
    out = tmp_path / 'hybrid.png'
    (tmp_path / 'grey_scenes.py').write_text(GREY_SCENES)
    env = dict(os.environ, HOME=str(tmp_path))
    proc = subprocess.run([sys.executable, os.path.join(ROOT, 'bin', 'chroma-render'), '@grey_scenes.grey_tiny', '-r', '%d,%d' % size,
                           '--hybrid', '-s', str(seed), '-o', str(out)], cwd=str(tmp_path), env=env, capture_output=True,
                          text=True, timeout=600)
    assert proc.returncode == 0, proc.stderr[-3000:]
    w, h, rgb = _png_pixels(out.read_bytes())
    r, source = _renderer(_scene('grey_tiny'), size, seed=seed)
    want = r.snapshot(source).reshape(size[0], size[1]).T
    assert (want != 0xFF000000).sum() > 0.01 * want.size
    assert (w, h) == size
    assert np.array_equal(rgb[..., 0], (want >> 16) & 0xFF) and np.array_equal(rgb[..., 1], (want >> 8) & 0xFF) \
        and np.array_equal(rgb[..., 2], want & 0xFF)


@pytest.mark.timeout(300)
def test_bad_arguments_are_refused_before_any_launch():
    from conftest import make_stress_geometry
    from chroma_amd import _lib
    from chroma_amd.gpu.tools import zeros
    from chroma_amd.gpu import vec
    geometry = make_stress_geometry()
    r, source = _renderer(geometry, (8, 8), source_inside=(37.0, -210.0, 55.0))
    good1 = r.xyz_lookup1_gpu
    r.xyz_lookup1_gpu = zeros(r.ntriangles - 1, vec.float3, r.ctx)
    with pytest.raises(_lib.ChromaError):
        r.lookup_pass(r.npixels, r.ntriangles, 0, source, 545.0, (0, 1, 0))
    with pytest.raises(_lib.ChromaError):
        r.nlookup_calls = 1
        r.image_pass(545.0, (0, 1, 0))
    r.xyz_lookup1_gpu = good1
    r.max_steps = -1
    with pytest.raises(_lib.ChromaError):
        r.lookup_pass(r.npixels, r.ntriangles, 0, source, 545.0, (0, 1, 0))
    with pytest.raises(_lib.ChromaError):
        r.image_pass(545.0, (0, 1, 0))
    r.max_steps = 10
    with pytest.raises(_lib.ChromaError):           # more threads than draw counters
        r.lookup_pass(r.npixels + 1, r.ntriangles, 0, source, 545.0, (0, 1, 0))
    good_image = r.image_gpu
    r.image_gpu = zeros(r.npixels - 1, vec.float3, r.ctx)
    with pytest.raises(_lib.ChromaError):
        r.image_pass(545.0, (0, 1, 0))
    r.image_gpu = good_image
    r.nimages = 0
    with pytest.raises(_lib.ChromaError):
        r.process_image()
    r.ctx.synchronize()
    assert (r.rng_counters.get() == 0).all()
    assert not r.xyz_lookup1_gpu.get().view(f32).any() and not r.xyz_lookup2_gpu.get().view(f32).any()
    assert not r.image_gpu.get().view(f32).any() and not r.pixels_gpu.get().any()
