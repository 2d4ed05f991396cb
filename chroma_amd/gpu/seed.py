"""The vertex seed on the device (chroma_vertex_seed): ``GPUVertexSeeder`` keeps a ``chroma_amd.seed.VertexSeeder``'s channel
positions and candidates resident and runs whole batches of fits in one call.  The hit rows are uploaded per call -- a few MB at
the most; the work is in the (fit, candidate, hit) evaluations.  ``GPUDirectionSeeder`` does the same for a
``chroma_amd.seed.DirectionSeeder`` (chroma_direction_seed), and takes the hit rows, the positions and the bins of the vertex seed
that ran just before as they lie on the device."""
import ctypes

import numpy as np

from chroma_amd import _lib
from chroma_amd.gpu.tools import Context, get_context, to_gpu, zeros


class GPUVertexSeeder(object):
    """``where``: a context, or anything made on one (a ``GPUDetector``, a ``GPUGeometry``: its ``ctx``), or None for the
    current context.  ``fit_many`` / ``fit`` are the seeder's own with ``gpu=self``."""

    def __init__(self, where, seeder):
        ctx = where if isinstance(where, Context) else getattr(where, 'ctx', None)
        self.ctx = ctx if ctx is not None else get_context()
        self.seeder = seeder
        self.channel_pos = to_gpu(seeder.channel_pos.reshape(-1), ctx=self.ctx) if seeder.nchannels else None
        self.cand = to_gpu(seeder.cand.reshape(-1), ctx=self.ctx)

    def run(self, prepared, scores=False, keep=False):
        """chroma_vertex_seed on ``prepared`` (``VertexSeeder.prepare``): the output arrays of ``VertexSeeder.run_host``, read back.
        ``keep``: (those, the call's device arrays {'hits': [channel, time, weight], 'best_pos', 'best_bin'} or None without fits),
        for ``GPUDirectionSeeder.run(..., device=...)``."""
        s, ctx, n = self.seeder, self.ctx, prepared.nfits
        out = s.outputs(n, scores)
        if n == 0:
            return (out, None) if keep else out
        hits = [to_gpu(a, ctx=ctx) if len(a) else None for a in (prepared.channel, prepared.time, prepared.weight)]
        d_out = [None if a is None else zeros(a.size, a.dtype, ctx=ctx) for a in out]
        p = lambda a: None if a is None else ctypes.c_void_p(a.ptr)
        _lib.check(ctx._lib.chroma_vertex_seed(ctx.handle, ctypes.byref(prepared.struct), s.nchannels, p(self.channel_pos), len(s.cand), p(self.cand), n,
                                               _lib.ptr(prepared.offsets), _lib.ptr(prepared.tau0), *([p(a) for a in hits] + [p(a) for a in d_out])),
                   ctx._lib)
        back = [None if a is None else d.get().reshape(a.shape) for a, d in zip(out, d_out)]
        return (back, dict(hits=hits, best_pos=d_out[0], best_bin=d_out[2])) if keep else back

    def fit_many(self, offsets, channel, t_ns, weight=None, scores=False):
        return self.seeder.fit_many(offsets, channel, t_ns, weight, gpu=self, scores=scores)

    def fit(self, channel, t_ns, weight=None, scores=False):
        return self.seeder.fit(channel, t_ns, weight, gpu=self, scores=scores)


class GPUDirectionSeeder(object):
    """``where`` as ``GPUVertexSeeder``'s; ``seeder`` a ``chroma_amd.seed.DirectionSeeder``: its candidates and its vertex seeder's
    channel positions stay resident (``vertex``: a ``GPUVertexSeeder`` of that vertex seeder on the same context lends its copy)."""

    def __init__(self, where, seeder, vertex=None):
        ctx = where if isinstance(where, Context) else getattr(where, 'ctx', None)
        self.ctx = ctx if ctx is not None else get_context()
        self.seeder = seeder
        v = seeder.vertex_seeder
        if vertex is not None and vertex.seeder is v and vertex.ctx is self.ctx:
            self.channel_pos = vertex.channel_pos
        else:
            self.channel_pos = to_gpu(v.channel_pos.reshape(-1), ctx=self.ctx) if v.nchannels else None
        self.cand = to_gpu(seeder.cand.reshape(-1), ctx=self.ctx)

    def run(self, prepared, cos_hist=False, device=None):
        """chroma_direction_seed on ``prepared`` (``DirectionSeeder.prepare``): the output arrays of ``DirectionSeeder.run_host``, read
        back.  ``device``: what ``GPUVertexSeeder.run(..., keep=True)`` kept of the vertex seed of the same rows -- the hit rows,
        the positions and the bins are then taken where they lie, not uploaded."""
        s, ctx, n = self.seeder, self.ctx, prepared.nfits
        out = s.outputs(n, cos_hist)
        if n == 0:
            return out
        if device is None:
            hits = [None if a is None or not len(a) else to_gpu(a, ctx=ctx) for a in (prepared.channel, prepared.time, prepared.weight)]
            vertex, bin = to_gpu(prepared.vertex.reshape(-1), ctx=ctx), to_gpu(prepared.bin, ctx=ctx)
        else:
            hits = list(device['hits'])
            vertex, bin = device['best_pos'], device['best_bin']
            if prepared.time is None:
                hits[1] = None
        d_out = [None if a is None else zeros(a.size, a.dtype, ctx=ctx) for a in out]
        p = lambda a: None if a is None else ctypes.c_void_p(a.ptr)
        _lib.check(ctx._lib.chroma_direction_seed(ctx.handle, ctypes.byref(prepared.struct), ctypes.byref(prepared.timing), s.vertex_seeder.nchannels,
                                                  p(self.channel_pos), len(s.cand), p(self.cand), n, _lib.ptr(prepared.offsets), _lib.ptr(prepared.tau0),
                                                  p(vertex), p(bin), *([p(a) for a in hits] + [p(a) for a in d_out])), ctx._lib)
        return [None if a is None else d.get().reshape(a.shape) for a, d in zip(out, d_out)]

    def fit_many(self, seed_fits, offsets, channel, t_ns=None, weight=None, cos_hist=False):
        return self.seeder.fit_many(seed_fits, offsets, channel, t_ns, weight, gpu=self, cos_hist=cos_hist)

    def fit(self, seed_fits, channel, t_ns=None, weight=None, cos_hist=False):
        return self.seeder.fit(seed_fits, channel, t_ns, weight, gpu=self, cos_hist=cos_hist)

    def fit_both(self, vertex, offsets, channel, t_ns, weight=None, cos_hist=False):
        """(``SeedFits``, ``DirFits``) of the rows: the vertex seed on ``vertex`` (a ``GPUVertexSeeder`` of this seeder's vertex
        seeder), then the direction seed about it with the rows, positions and bins handed over on the device -- the bits of
        ``fit_many`` one after the other."""
        v = self.seeder.vertex_seeder
        if vertex.seeder is not v:
            raise ValueError('the GPUVertexSeeder was made for another seeder')
        prepared = v.prepare(offsets, channel, t_ns, weight)
        out, device = vertex.run(prepared, keep=True)
        seed_fits = v.finish(prepared, out)
        about = self.seeder.prepare(seed_fits, offsets, channel, t_ns, weight, prepared=prepared)
        return seed_fits, self.seeder.finish(about, self.run(about, cos_hist, device=device))
