"""Photons from the step points of charged particles, made ON THE DEVICE (chroma_steps_count / chroma_steps_generate, and
chroma_steps_count_media / chroma_steps_generate_media with a medium per segment).

``LightSource``, ``LightMedia`` and ``segments_from_vertices`` are those of ``chroma_amd.generator.steps`` (NumPy; see there
for the physics and for what is read of a Material -- ``scintillation_rise_time`` and ``scintillation_mod`` are not, and
``qedep`` is taken as already quenched).  ``generate_photons`` uploads the segments (48 bytes each), counts, scans and
generates on the context's stream, and returns the photons as device arrays ready for ``propagate`` / ``propagate_hits``: they
never visit the host.  The same segments, seed and ``segment_base`` give, bit for bit, the photons of the host generator.

With a ``LightMedia`` every segment emits the light of the medium it lies in.  Which one that is the caller says
(``medium``), or the device finds out: ``locate_materials`` casts one ray from each segment's midpoint through the geometry
and reads the material off the first triangle it meets (chroma_locate_materials).
"""
import ctypes
import weakref

import numpy as np

from chroma_amd import _lib
from chroma_amd.generator.steps import LightSource, LightMedia, Segments, segments_from_vertices, _as_segments, _SEGMENT_FIELDS
from chroma_amd.gpu.tools import GPUArray, get_context, empty, to_gpu
from chroma_amd.gpu.photon import GPUPhotonsSlice, _alloc_fields, _structure

__all__ = ['LightSource', 'LightMedia', 'Segments', 'segments_from_vertices', 'generate_photons', 'locate_materials', 'segment_midpoints']


def locate_materials(points, gpu_geometry, direction=None, outside=-1, return_triangles=False):
    """The material index (into ``geometry.unique_materials``) of the solid each of ``points`` lies in: a GPUArray (int32) in
    point order.  ``points``: a host array (n, 3) or a GPUArray of 3 n float32.  One ray per point along ``direction``
    (default (0, 0, 1)) meets its nearest triangle, and the side of that triangle the point is on names the material, by the
    rule a photon starting there would get its first medium by (``fill_state``); a ray that meets nothing gives ``outside``.
    A probe direction that is parallel to an axis is cast by the strict walk alone and costs several times a generic one.
    ``return_triangles``: also the deciding triangle of each point (-1: none), what ``intersect_mesh`` returns for the ray."""
    ctx = gpu_geometry.ctx
    if not isinstance(points, GPUArray):
        points = to_gpu(np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3).reshape(-1), ctx)
    if points.size % 3:
        raise ValueError('points: 3 floats each')
    n = points.size // 3
    if direction is not None:
        direction = (ctypes.c_float * 3)(*[float(x) for x in direction])
    material = empty(n, np.int32, ctx)
    triangles = empty(n, np.int32, ctx) if return_triangles else None
    _lib.check(ctx._lib.chroma_locate_materials(ctx.handle, gpu_geometry.handle, n, points.ptr, direction, int(outside), material.ptr,
                                                triangles.ptr if return_triangles else None), ctx._lib)
    return (material, triangles) if return_triangles else material


def segment_midpoints(segments):
    """float32 (n, 3): ``0.5f * (a + b)`` in single precision, the point a segment's medium is looked up at."""
    return np.float32(0.5) * (segments.a + segments.b)


class _DeviceMedia(object):
    """chroma_light_media of one LightMedia on one context"""

    def __init__(self, media, ctx):
        self.lib = ctx._lib
        self.handle = ctypes.c_void_p()
        _lib.check(self.lib.chroma_light_media_create(ctx.handle, ctypes.byref(media.desc), ctypes.byref(self.handle)), self.lib)

    def destroy(self):
        if self.handle is not None and self.handle.value:
            handle, self.handle = self.handle, None
            try:
                self.lib.chroma_light_media_destroy(handle)
            except Exception:   # interpreter shutdown
                pass


def device_media(media, ctx):
    """The device-resident table of ``media`` on ``ctx``: made at first use, kept by the context, and destroyed with the
    LightMedia or at the context's shutdown(), whichever comes first."""
    owned = ctx.__dict__.setdefault('_light_media', {})
    entry = owned.get(id(media))
    if entry is None:
        entry = owned[id(media)] = _DeviceMedia(media, ctx)
        weakref.finalize(media, _drop_media, weakref.ref(ctx), id(media))
    return entry


def _drop_media(ctx_ref, key):
    ctx = ctx_ref()
    entry = ctx.__dict__.get('_light_media', {}).pop(key, None) if ctx is not None else None
    if entry is not None:
        entry.destroy()


def generate_photons(vertices_or_segments, source, seed, ctx=None, evidx=0, segment_base=0, return_offsets=False, medium=None,
                     gpu_geometry=None, outside=-1, return_medium=False):
    """The photons ``source`` emits along the segments (a Segments, the vertices whose steps make them, or the
    ``gpu.particles.DeviceSegments`` of tracks made on the device, whose own ``medium`` is the default): a GPUPhotonsSlice
    in segment order, a segment's Cherenkov photons before its scintillation photons; ``evidx`` follows the segment,
    ``rng_counters`` is 0.  ``return_offsets``: also the scanned counts as a host array (uint32, 2 n + 1: the photons of segment
    s are ``offsets[2 s] .. offsets[2 s + 2]``).

    ``source`` is a LightSource, one medium for all segments, or a LightMedia.  Then segment s emits the light of row
    ``medium[s]`` (an int array on the host, or a GPUArray of int32; a row outside the table emits nothing); with
    ``medium=None`` and a ``gpu_geometry`` the rows are the materials the segments' midpoints lie in, found on the device
    (``locate_materials``; ``outside``: the row of a segment outside every solid) -- the media are then those of
    ``LightMedia.from_geometry``.  The located rows go into the count and generate calls where they are; ``return_medium``:
    also that GPUArray."""
    ctx = ctx or (gpu_geometry.ctx if gpu_geometry is not None else getattr(vertices_or_segments, 'ctx', None) or get_context())
    lib = ctx._lib
    seed = int(seed) & (2 ** 64 - 1)
    from chroma_amd.gpu.particles import DeviceSegments
    if isinstance(vertices_or_segments, DeviceSegments):
        # (segments the particle stepper left on the device, with the medium each was made in: used where they are)
        segments, seg = vertices_or_segments, vertices_or_segments.struct()
        if medium is None:
            medium = segments.medium[:len(segments)]
    else:
        segments = _as_segments(vertices_or_segments, evidx, segment_base)
        device = {name: to_gpu(getattr(segments, name).reshape(-1), ctx) for name in _SEGMENT_FIELDS}
        seg = segments.struct({name: a.ptr for name, a in device.items()})
    d_offsets = empty(2 * len(segments) + 1, np.uint32, ctx)
    total = ctypes.c_uint64()
    if isinstance(source, LightMedia):
        if medium is None:
            if gpu_geometry is None:
                raise ValueError('a LightMedia needs medium=, or gpu_geometry= to find it in')
            if gpu_geometry.ctx is not ctx:
                raise ValueError('gpu_geometry belongs to another context')
            medium = locate_materials(segment_midpoints(segments), gpu_geometry, outside=outside)
        elif not isinstance(medium, GPUArray):
            medium = to_gpu(np.ascontiguousarray(np.broadcast_to(np.asarray(medium, dtype=np.int32), (len(segments),))), ctx)
        if medium.size != len(segments) or medium.dtype != np.int32:
            raise ValueError('medium: one int32 per segment')
        table = device_media(source, ctx)
        _lib.check(lib.chroma_steps_count_media(ctx.handle, table.handle, ctypes.byref(seg), medium.ptr, seed, d_offsets.ptr,
                                                ctypes.byref(total)), lib)
    else:
        if medium is not None or return_medium:
            raise ValueError('medium= goes with a LightMedia, not with one LightSource')
        _lib.check(lib.chroma_steps_count(ctx.handle, ctypes.byref(source.struct), ctypes.byref(seg), seed, d_offsets.ptr,
                                          ctypes.byref(total)), lib)
    n = total.value
    out = GPUPhotonsSlice(rng_counters=empty(n, np.uint32, ctx), **_alloc_fields(n, ctx))
    arrays = _structure(out)
    if isinstance(source, LightMedia):
        _lib.check(lib.chroma_steps_generate_media(ctx.handle, table.handle, ctypes.byref(seg), medium.ptr, seed, d_offsets.ptr,
                                                   ctypes.byref(arrays), n), lib)
    else:
        _lib.check(lib.chroma_steps_generate(ctx.handle, ctypes.byref(source.struct), ctypes.byref(seg), seed, d_offsets.ptr,
                                             ctypes.byref(arrays), n), lib)
    result = (out,)
    if return_offsets:
        result += (d_offsets.get(),)
    if return_medium:
        result += (medium,)
    return result if len(result) > 1 else out
