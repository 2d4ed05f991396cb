"""GPURays: ray bundles on the device and the `render` kernel (reference: chroma/gpu/render.py:7-66).

Same constructor, methods and arguments; the transforms and the render call go through the C ABI
(chroma_points_translate / _rotate / _rotate_around_point, chroma_render) instead of PyCUDA kernels looked
up by name.  ``nblocks`` (threads per block in the reference) is accepted and ignored.
"""
import ctypes

import numpy as np

from chroma_amd import _lib
from chroma_amd.gpu.tools import GPUArray, get_context, to_float3, to_gpu, zeros, empty, vec

float4 = np.dtype([('x', np.float32), ('y', np.float32), ('z', np.float32), ('w', np.float32)])


def _f3(v):
    return (ctypes.c_float * 3)(*[float(x) for x in v])


class GPURays(object):
    """The GPURays class holds arrays of ray positions and directions
    on the GPU that are used to render a geometry."""

    def __init__(self, pos, dir, max_alpha_depth=10, nblocks=64):
        self.ctx = get_context()
        self.pos = to_gpu(to_float3(pos), self.ctx)
        self.dir = to_gpu(to_float3(dir), self.ctx)
        self.max_alpha_depth = max_alpha_depth
        self.nblocks = nblocks
        self.dx = empty(max_alpha_depth * self.pos.size, np.float32, self.ctx)
        self.color = empty(self.dx.size, float4, self.ctx)
        self.dxlen = zeros(self.pos.size, np.uint32, self.ctx)

    def rotate(self, phi, n):
        "Rotate by an angle phi around the axis `n`."
        lib, h = self.ctx._lib, self.ctx.handle
        _lib.check(lib.chroma_points_rotate(h, self.pos.size, self.pos.ptr, float(phi), _f3(n)))
        _lib.check(lib.chroma_points_rotate(h, self.dir.size, self.dir.ptr, float(phi), _f3(n)))

    def rotate_around_point(self, phi, n, point):
        """"Rotate by an angle phi around the axis `n` passing through
        the point `point`."""
        lib, h = self.ctx._lib, self.ctx.handle
        _lib.check(lib.chroma_points_rotate_around_point(h, self.pos.size, self.pos.ptr, float(phi), _f3(n), _f3(point)))
        _lib.check(lib.chroma_points_rotate(h, self.dir.size, self.dir.ptr, float(phi), _f3(n)))

    def translate(self, v):
        "Translate the ray positions by the vector `v`."
        _lib.check(self.ctx._lib.chroma_points_translate(self.ctx.handle, self.pos.size, self.pos.ptr, _f3(v)))

    def render(self, gpu_geometry, pixels, alpha_depth=10, keep_last_render=False, bg_color=0x00000000):
        """Render `gpu_geometry` and fill the GPU array `pixels` with pixel
        colors."""
        if not keep_last_render:
            self.dxlen.fill(0)
        if alpha_depth > self.max_alpha_depth:
            raise Exception('alpha_depth > max_alpha_depth')
        if not isinstance(pixels, GPUArray):
            raise TypeError('`pixels` must be a %s instance.' % GPUArray)
        if pixels.size != self.pos.size:
            raise ValueError('`pixels`.size != number of rays')
        _lib.check(self.ctx._lib.chroma_render(self.ctx.handle, gpu_geometry.gpudata, self.pos.size, self.pos.ptr, self.dir.ptr,
                                               int(alpha_depth), pixels.ptr, self.dx.ptr, self.dxlen.ptr, self.color.ptr,
                                               int(bg_color) & 0xFFFFFFFF))

    def snapshot(self, gpu_geometry, alpha_depth=10):
        "Render `gpu_geometry` and return a numpy array of pixel colors."
        pixels = empty(self.pos.size, np.uint32, self.ctx)
        self.render(gpu_geometry, pixels, alpha_depth)
        return pixels.get()


# ---- the hybrid render (chroma/camera.py:188-249 over chroma/cuda/hybrid_render.cu) ----------------------------------------
# The host arithmetic of the mode, in plain NumPy (the tests restate the device results with it).
HYBRID_COLORS = ((685.0, (1, 0, 0)), (545.0, (0, 1, 0)), (445.0, (0, 0, 1)))      # (wavelength, xyz) as camera.py:214,231


def hybrid_chunks(ntriangles, npixels):
    """The (nthreads, total_threads, offset) of the lookup launches of one wavelength (camera.py:215-217): ntriangles // npixels
    + 1 chunks of npixels triangles, the last one partly (or wholly) past the last triangle."""
    return [(int(npixels), int(ntriangles), i * int(npixels)) for i in range(int(ntriangles) // int(npixels) + 1)]


def hybrid_accumulate(lookup1, lookup2, triangles, sides, contributions):
    """What one lookup launch adds to the tables, restated: the contributions (float32 [n][3], cos_theta * xyz) of
    the samples that diffused (triangle >= 0) are summed per (triangle, side) in sample order in f32, and each sum is added
    once to its entry of ``lookup1`` (side 1, inside to outside) or ``lookup2``.  The [ntriangles][3] float32 tables are
    updated in place and returned."""
    tri = np.asarray(triangles, np.int64).reshape(-1)
    side = np.asarray(sides, np.int64).reshape(-1)
    c = np.asarray(contributions, np.float32).reshape(-1, 3)
    sel = np.flatnonzero(tri >= 0)
    if len(sel) == 0:
        return lookup1, lookup2
    keys = 2 * tri[sel] + side[sel]
    perm = np.argsort(keys, kind='stable')
    order, skeys = sel[perm], keys[perm]
    starts = np.flatnonzero(np.r_[True, skeys[1:] != skeys[:-1]])
    lengths = np.diff(np.r_[starts, len(skeys)])
    sums = c[order[starts]].copy()
    for m in range(1, int(lengths.max())):
        more = lengths > m
        sums[more] = sums[more] + c[order[starts[more] + m]]
    seg = skeys[starts]
    for s, table in ((1, lookup1), (0, lookup2)):
        on = (seg & 1) == s
        t = seg[on] >> 1
        table[t] = table[t] + sums[on]
    return lookup1, lookup2


def hybrid_image_update(image, triangles, sides, lookup1, lookup2, xyz, nlookup_calls):
    """update_xyz_image's addition restated: image[k] += xyz * lookup[triangle] / nlookup_calls for the rays that diffused
    (float3 operation order of hybrid_render.cu:161-165).  ``image`` [n][3] float32 is updated in place and returned."""
    tri = np.asarray(triangles, np.int64).reshape(-1)
    side = np.asarray(sides).reshape(-1)
    sel = np.flatnonzero(tri >= 0)
    look = np.where((side[sel] == 1)[:, None], lookup1[tri[sel]], lookup2[tri[sel]]).astype(np.float32)
    image[sel] = image[sel] + (np.asarray(xyz, np.float32)[None, :] * look) / np.float32(nlookup_calls)
    return image


def hybrid_pixels(image, nimages):
    """process_image (hybrid_render.cu:170-201): image / nimages, each channel clamped to [0, 1] (NaN to 0), floorf(x * 255),
    packed 0xFF << 24 | r << 16 | g << 8 | b (uint32)."""
    rgb = np.asarray(image, np.float32).reshape(-1, 3) / np.float32(nimages)
    rgb = np.where(rgb >= np.float32(0), rgb, np.float32(0))
    rgb = np.where(rgb > np.float32(1), np.float32(1), rgb)
    ch = np.floor(rgb * np.float32(255)).astype(np.uint32)
    return (np.uint32(0xFF << 24) | ch[:, 0] << np.uint32(16) | ch[:, 1] << np.uint32(8) | ch[:, 2]).astype(np.uint32)


def png_bytes(pixels, width, height):
    """An 8-bit RGB PNG of ``pixels`` (uint32 0xAARRGGBB, alpha dropped) in the order from_film lays rays out: ray
    x * height + y is column x, row y (pygame.surfarray's [x][y], the camera's display).  Standard library only."""
    import struct
    import zlib
    p = np.asarray(pixels, np.uint32).reshape(int(width), int(height)).T
    rgb = np.stack([(p >> 16) & 0xFF, (p >> 8) & 0xFF, p & 0xFF], axis=-1).astype(np.uint8)
    raw = b''.join(b'\x00' + row.tobytes() for row in rgb)

    def chunk(kind, data):
        return struct.pack('>I', len(data)) + kind + data + struct.pack('>I', zlib.crc32(kind + data) & 0xFFFFFFFF)
    return (b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', int(width), int(height), 8, 2, 0, 0, 0))
            + chunk(b'IDAT', zlib.compress(raw, 6)) + chunk(b'IEND', b''))


def write_png(path, pixels, width, height):
    with open(path, 'wb') as f:
        f.write(png_bytes(pixels, width, height))


def _ptr_or_none(a):
    return None if a is None else a.ptr


class GPUHybridRender(object):
    """The camera's "hybrid" mode without a display (chroma/camera.py:188-249): light the geometry from a point source
    with the real optics.  ``update_xyz_lookup`` sends photons from the source to every triangle and records, per triangle
    and side, where they first reflect diffusely; ``update_image`` sends one photon per camera ray to its first diffuse
    reflection and reads the table there; ``process_image`` turns the accumulated image into pixels.

    ``rays`` is a GPURays bundle (one ray per pixel).  The state keeps Camera's names.  The draw counters
    (``rng_counters``, one per pixel, shared by both passes as the reference's rng_states) continue from call to call."""

    def __init__(self, gpu_geometry, rays, seed=None, max_steps=10):
        from chroma_amd.sim import pick_seed
        self.ctx = rays.ctx
        self.gpu_geometry = gpu_geometry
        self.rays = rays
        self.npixels = rays.pos.size
        self.ntriangles = gpu_geometry.triangles.size
        self.seed = pick_seed() if seed is None else int(seed)
        self.rng = _lib.Rng(self.seed & 0xFFFFFFFFFFFFFFFF, 0)
        self.rng_counters = zeros(self.npixels, np.uint32, self.ctx)
        self.max_steps = int(max_steps)
        self.xyz_lookup1_gpu = zeros(self.ntriangles, vec.float3, self.ctx)
        self.xyz_lookup2_gpu = zeros(self.ntriangles, vec.float3, self.ctx)
        self.image_gpu = zeros(self.npixels, vec.float3, self.ctx)
        self.pixels_gpu = zeros(self.npixels, np.uint32, self.ctx)
        self.nlookup_calls = 0
        self.nimages = 0

    def clear_xyz_lookup(self):
        self.xyz_lookup1_gpu.fill(vec.make_float3(0.0, 0.0, 0.0))
        self.xyz_lookup2_gpu.fill(vec.make_float3(0.0, 0.0, 0.0))
        self.nlookup_calls = 0

    def lookup_pass(self, nthreads, total_threads, offset, source_position, wavelength, xyz, samples=None):
        """One update_xyz_lookup launch.  ``samples``: optional (triangle int32, side uint32, history uint32, cos_theta float32)
        GPUArrays of ``nthreads`` entries for the per-sample outputs."""
        s = samples if samples is not None else (None,) * 4
        _lib.check(self.ctx._lib.chroma_hybrid_lookup(
            self.ctx.handle, self.gpu_geometry.gpudata, int(nthreads), int(total_threads), int(offset), _f3(source_position),
            self.rng, self.rng_counters.ptr, self.rng_counters.size, float(wavelength), _f3(xyz), self.xyz_lookup1_gpu.ptr,
            self.xyz_lookup2_gpu.ptr, min(self.xyz_lookup1_gpu.size, self.xyz_lookup2_gpu.size), self.max_steps,
            *[_ptr_or_none(a) for a in s]))

    def update_xyz_lookup(self, source_position):
        for wavelength, xyz in HYBRID_COLORS:
            for nthreads, total, offset in hybrid_chunks(self.ntriangles, self.npixels):
                self.lookup_pass(nthreads, total, offset, source_position, wavelength, xyz)
        self.nlookup_calls += 1

    def clear_image(self):
        self.image_gpu.fill(vec.make_float3(0.0, 0.0, 0.0))
        self.nimages = 0

    def image_pass(self, wavelength, xyz, samples=None):
        """One update_xyz_image launch over all rays (``samples``: optional triangle, side, history GPUArrays)."""
        s = samples if samples is not None else (None,) * 3
        _lib.check(self.ctx._lib.chroma_hybrid_image(
            self.ctx.handle, self.gpu_geometry.gpudata, self.rays.pos.size, self.rng, self.rng_counters.ptr, self.rng_counters.size,
            self.rays.pos.ptr, self.rays.dir.ptr, float(wavelength), _f3(xyz), self.xyz_lookup1_gpu.ptr, self.xyz_lookup2_gpu.ptr,
            min(self.xyz_lookup1_gpu.size, self.xyz_lookup2_gpu.size), self.image_gpu.ptr, self.image_gpu.size,
            int(self.nlookup_calls), self.max_steps, *[_ptr_or_none(a) for a in s]))

    def update_image(self):
        for wavelength, xyz in HYBRID_COLORS:
            self.image_pass(wavelength, xyz)
        self.nimages += 1

    def process_image(self):
        if self.pixels_gpu.size != self.image_gpu.size:
            raise ValueError('pixels and image differ in size')
        _lib.check(self.ctx._lib.chroma_hybrid_pixels(self.ctx.handle, self.image_gpu.size, self.image_gpu.ptr, self.pixels_gpu.ptr,
                                                      int(self.nimages)))

    def snapshot(self, source_position, nlookup=1, nimages=1):
        """Fresh tables and image, ``nlookup`` lookup passes from ``source_position``, ``nimages`` image passes; the pixels
        (host uint32, 0xAARRGGBB, one per ray)."""
        self.clear_xyz_lookup()
        for _ in range(int(nlookup)):
            self.update_xyz_lookup(source_position)
        self.clear_image()
        for _ in range(int(nimages)):
            self.update_image()
        self.process_image()
        return self.pixels_gpu.get()
