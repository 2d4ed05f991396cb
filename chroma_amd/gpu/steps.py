"""Photons from the step points of charged particles, made ON THE DEVICE (chroma_steps_count / chroma_steps_generate).

``LightSource`` and ``segments_from_vertices`` are those of ``chroma_amd.generator.steps`` (NumPy; see there for the
physics and for what is read of a Material -- ``scintillation_rise_time`` and ``scintillation_mod`` are not, and ``qedep``
is taken as already quenched).  ``generate_photons`` uploads the segments (48 bytes each), counts, scans and generates
on the context's stream, and returns the photons as device arrays ready for ``propagate`` / ``propagate_hits``: they never
visit the host.  The same segments, seed and ``segment_base`` give, bit for bit, the photons of the host generator.
"""
import ctypes

import numpy as np

from chroma_amd import _lib
from chroma_amd.generator.steps import LightSource, Segments, segments_from_vertices, _as_segments, _SEGMENT_FIELDS
from chroma_amd.gpu.tools import get_context, empty, to_gpu
from chroma_amd.gpu.photon import GPUPhotonsSlice, _alloc_fields, _structure

__all__ = ['LightSource', 'Segments', 'segments_from_vertices', 'generate_photons']


def generate_photons(vertices_or_segments, source, seed, ctx=None, evidx=0, segment_base=0, return_offsets=False):
    """The photons ``source`` (a LightSource) emits along the segments (a Segments, or the vertices whose steps make them):
    a GPUPhotonsSlice in segment order, a segment's Cherenkov photons before its scintillation photons; ``evidx`` follows
    the segment, ``rng_counters`` is 0.  ``return_offsets``: also the scanned counts as a host array (uint32, 2 n + 1: the
    photons of segment s are ``offsets[2 s] .. offsets[2 s + 2]``)."""
    ctx = ctx or get_context()
    lib = ctx._lib
    segments = _as_segments(vertices_or_segments, evidx, segment_base)
    seed = int(seed) & (2 ** 64 - 1)
    device = {name: to_gpu(getattr(segments, name).reshape(-1), ctx) for name in _SEGMENT_FIELDS}
    seg = segments.struct({name: a.ptr for name, a in device.items()})
    d_offsets = empty(2 * len(segments) + 1, np.uint32, ctx)
    total = ctypes.c_uint64()
    _lib.check(lib.chroma_steps_count(ctx.handle, ctypes.byref(source.struct), ctypes.byref(seg), seed, d_offsets.ptr,
                                      ctypes.byref(total)), lib)
    n = total.value
    out = GPUPhotonsSlice(rng_counters=empty(n, np.uint32, ctx), **_alloc_fields(n, ctx))
    arrays = _structure(out)
    _lib.check(lib.chroma_steps_generate(ctx.handle, ctypes.byref(source.struct), ctypes.byref(seg), seed, d_offsets.ptr,
                                         ctypes.byref(arrays), n), lib)
    if return_offsets:
        return out, d_offsets.get()
    return out
