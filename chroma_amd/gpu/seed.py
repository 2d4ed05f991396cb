"""The vertex seed on the device (chroma_vertex_seed): ``GPUVertexSeeder`` keeps a ``chroma_amd.seed.VertexSeeder``'s channel
positions and candidates resident and runs whole batches of fits in one call.  The hit rows are uploaded per call -- a few MB at
the most; the work is in the (fit, candidate, hit) evaluations."""
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

    def run(self, prepared, scores=False):
        """chroma_vertex_seed on ``prepared`` (``VertexSeeder.prepare``): the output arrays of ``VertexSeeder.run_host``, read back."""
        s, ctx, n = self.seeder, self.ctx, prepared.nfits
        out = s.outputs(n, scores)
        if n == 0:
            return out
        hits = [to_gpu(a, ctx=ctx) if len(a) else None for a in (prepared.channel, prepared.time, prepared.weight)]
        d_out = [None if a is None else zeros(a.size, a.dtype, ctx=ctx) for a in out]
        p = lambda a: None if a is None else ctypes.c_void_p(a.ptr)
        _lib.check(ctx._lib.chroma_vertex_seed(ctx.handle, ctypes.byref(prepared.struct), s.nchannels, p(self.channel_pos), len(s.cand), p(self.cand), n,
                                               _lib.ptr(prepared.offsets), _lib.ptr(prepared.tau0), *([p(a) for a in hits] + [p(a) for a in d_out])),
                   ctx._lib)
        return [None if a is None else d.get().reshape(a.shape) for a, d in zip(out, d_out)]

    def fit_many(self, offsets, channel, t_ns, weight=None, scores=False):
        return self.seeder.fit_many(offsets, channel, t_ns, weight, gpu=self, scores=scores)

    def fit(self, channel, t_ns, weight=None, scores=False):
        return self.seeder.fit(channel, t_ns, weight, gpu=self, scores=scores)
