"""Charged particles stepped through the detector ON THE DEVICE (chroma_particles_track and the calls around it): the model,
``StoppingMedia``, ``Stepper`` and ``Tracks`` are those of ``chroma_amd.generator.particles`` (see there).

``track`` steps the vertices through a ``GPUGeometry`` -- every step is limited at the next triangle along the particle's
direction, found with the engine's ray cast, and made in the medium on the particle's side of that triangle -- or, without
a geometry, through one medium, which gives bit for bit the tracks of the host loop.  ``track_segments`` leaves the result on
the device as the segments and medium rows that ``chroma_amd.gpu.steps.generate_photons`` takes: nothing is read back.
"""
import ctypes
import weakref

import numpy as np

from chroma_amd import _lib
from chroma_amd.generator.particles import (StoppingMedia, Stepper, Tracks, ParticleState, POINT_FIELDS, point_struct, fill_steps,
                                            _as_list)
from chroma_amd.generator.steps import Segments, _SEGMENT_FIELDS
from chroma_amd.gpu.tools import GPUArray, get_context, empty, to_gpu

__all__ = ['StoppingMedia', 'Stepper', 'Tracks', 'DeviceSegments', 'device_stopping_media', 'track', 'track_segments']

_SEGMENT_TYPES = dict(a=(np.float32, 3), b=(np.float32, 3), t_a=(np.float32, 1), t_b=(np.float32, 1), beta=(np.float32, 1), z=(np.float32, 1),
                      qedep=(np.float32, 1), evidx=(np.uint32, 1))


class _DeviceStoppingMedia(object):
    """chroma_stopping_media of one StoppingMedia on one context"""

    def __init__(self, media, ctx):
        self.lib = ctx._lib
        self.handle = ctypes.c_void_p()
        _lib.check(self.lib.chroma_stopping_media_create(ctx.handle, ctypes.byref(media.desc), ctypes.byref(self.handle)), self.lib)

    def destroy(self):
        if self.handle is not None and self.handle.value:
            handle, self.handle = self.handle, None
            try:
                self.lib.chroma_stopping_media_destroy(handle)
            except Exception:   # interpreter shutdown
                pass


def device_stopping_media(media, ctx):
    """The device-resident table of ``media`` on ``ctx``: made at first use, kept by the context, and destroyed with the
    StoppingMedia or at the context's shutdown(), whichever comes first (as ``gpu.steps.device_media``)."""
    owned = ctx.__dict__.setdefault('_stopping_media', {})
    entry = owned.get(id(media))
    if entry is None:
        entry = owned[id(media)] = _DeviceStoppingMedia(media, ctx)
        weakref.finalize(media, _drop_media, weakref.ref(ctx), id(media))
    return entry


def _drop_media(ctx_ref, key):
    ctx = ctx_ref()
    entry = ctx.__dict__.get('_stopping_media', {}).pop(key, None) if ctx is not None else None
    if entry is not None:
        entry.destroy()


class DeviceSegments(object):
    """Segments as device arrays (the fields of ``generator.steps.Segments``, GPUArrays) and ``medium``, the row of each
    (int32).  ``gpu.steps.generate_photons`` takes one in place of a Segments."""

    def __init__(self, arrays, medium, n, segment_base=0, ctx=None):
        self.arrays, self.medium, self.n, self.segment_base, self.ctx = arrays, medium, int(n), int(segment_base), ctx

    def __len__(self):
        return self.n

    def struct(self):
        s = _lib.StepSegments()
        for name in _SEGMENT_FIELDS:
            setattr(s, name, self.arrays[name].ptr)
        s.n, s.segment_base = self.n, self.segment_base
        return s

    def get(self):
        """(Segments, medium) on the host."""
        host = {name: self.arrays[name].get()[:self.n * _SEGMENT_TYPES[name][1]] for name in _SEGMENT_FIELDS}
        return Segments(*[host[name] for name in _SEGMENT_FIELDS], segment_base=self.segment_base), self.medium.get()[:self.n]


class DeviceParticles(object):
    """The particles of one call on the device, and the chroma_particle_arrays over them"""

    def __init__(self, state, ctx):
        self.state, self.ctx = state, ctx
        self.arrays = {name: to_gpu(getattr(state, name).reshape(-1), ctx) for name, _ in ParticleState.FIELDS}
        self.struct = state.struct({name: a.ptr for name, a in self.arrays.items()})

    def fetch(self):
        """The device's values back into the host ParticleState."""
        for name, _ in ParticleState.FIELDS:
            setattr(self.state, name, self.arrays[name].get().reshape(getattr(self.state, name).shape))
        return self.state


def _device_points(rows, ctx):
    arrays = {name: empty(max(rows, 1) * width, dtype, ctx) for name, dtype, width in POINT_FIELDS}
    return arrays, point_struct({name: a.ptr for name, a in arrays.items()})


def _run(vertices, stepper, seed, gpu_geometry, ctx, particle_base, evidx, medium):
    ctx = ctx or (gpu_geometry.ctx if gpu_geometry is not None else get_context())
    if gpu_geometry is not None and gpu_geometry.ctx is not ctx:
        raise ValueError('gpu_geometry belongs to another context')
    if gpu_geometry is None and medium is None and stepper.outside < 0:
        raise ValueError('without a geometry the particles need a medium: medium=row, or Stepper(outside=row)')
    particles = DeviceParticles(ParticleState(vertices, evidx=evidx, particle_base=particle_base), ctx)
    options = stepper.options(outside=medium if gpu_geometry is None else None)
    table = device_stopping_media(stepper.media, ctx)
    total = ctypes.c_uint64()
    _lib.check(ctx._lib.chroma_particles_track(ctx.handle, gpu_geometry.handle if gpu_geometry is not None else None, table.handle,
                                               ctypes.byref(particles.struct), ctypes.byref(options), int(seed) & (2 ** 64 - 1),
                                               ctypes.byref(total)), ctx._lib)
    return ctx, particles, total.value


def track(vertices, stepper, seed, gpu_geometry=None, ctx=None, particle_base=0, evidx=0, medium=None):
    """The tracks of ``vertices`` made on the device: (the vertices with ``steps`` filled, copies; a Tracks).  With a
    ``gpu_geometry`` in its volumes, a medium row being a material index of the geometry (``StoppingMedia.from_geometry``) and
    ``stepper.outside`` the row around everything; without one in row ``medium`` for all, as ``generator.particles.track``."""
    vertices = _as_list(vertices)
    ctx, particles, total = _run(vertices, stepper, seed, gpu_geometry, ctx, particle_base, evidx, medium)
    points, struct = _device_points(total, ctx)
    d_offsets = empty(particles.state.n + 1, np.uint32, ctx)
    _lib.check(ctx._lib.chroma_particles_points(ctx.handle, ctypes.byref(struct), d_offsets.ptr, total), ctx._lib)
    flat = {name: points[name].get()[:total * width].reshape((total, width) if width > 1 else (total,)) for name, _, width in POINT_FIELDS}
    tracks = Tracks(flat, d_offsets.get(), particles.fetch())
    return fill_steps(vertices, tracks), tracks


def track_segments(vertices, stepper, seed, gpu_geometry=None, ctx=None, particle_base=0, evidx=0, medium=None, segment_base=0,
                   return_tracks=False):
    """The tracks as a DeviceSegments: made and cut into segments on the device, nothing read back but their number.
    ``return_tracks``: also (vertices with steps, Tracks), which does read the points back."""
    vertices = _as_list(vertices)
    ctx, particles, total = _run(vertices, stepper, seed, gpu_geometry, ctx, particle_base, evidx, medium)
    n = total - particles.state.n
    arrays = {name: empty(max(n, 1) * width, dtype, ctx) for name, (dtype, width) in _SEGMENT_TYPES.items()}
    d_medium = empty(max(n, 1), np.int32, ctx)
    out = DeviceSegments(arrays, d_medium, n, segment_base, ctx)
    seg = out.struct()
    _lib.check(ctx._lib.chroma_particles_segments(ctx.handle, ctypes.byref(seg), d_medium.ptr, n), ctx._lib)
    if not return_tracks:
        return out
    points, struct = _device_points(total, ctx)
    d_offsets = empty(particles.state.n + 1, np.uint32, ctx)
    _lib.check(ctx._lib.chroma_particles_points(ctx.handle, ctypes.byref(struct), d_offsets.ptr, total), ctx._lib)
    flat = {name: points[name].get()[:total * width].reshape((total, width) if width > 1 else (total,)) for name, _, width in POINT_FIELDS}
    tracks = Tracks(flat, d_offsets.get(), particles.fetch())
    return out, fill_steps(vertices, tracks), tracks
