"""GPUDaq / GPUChannels: per-channel earliest hit time, charge and history
(reference: chroma/gpu/daq.py:8-100 over chroma/cuda/daq.cu).

``ndaq == 1`` runs ``run_daq``; ``ndaq > 1`` runs ``run_daq_many`` (daq.cu:88-150): that many
independent acquisitions of the same photons side by side, each with a unit normal jitter on the hit
time (``GPUChannels.iterate_copies`` walks them).  The random numbers a detected photon consumes
(weight gate, jitter, time smear, charge) come from Philox stream ``1 + acquisition`` of that photon
(copy i from word 8 i on), so propagation draws are not disturbed and two acquisitions of the same
photons differ.

``GPUEventDaq`` runs the per-event acquisitions of a whole batch -- what ``Simulation.simulate(run_daq=True)`` asks for -- as one
acquisition over a row of channels per event and reads the touched words back sparse (``EventChannels``).
"""
import ctypes

import numpy as np

from chroma_amd import _lib, event
from chroma_amd.gpu.tools import GPUArray, get_context, empty, zeros, to_gpu, RNGStates
from chroma_amd.gpu.photon import _structure


class GPUChannels(object):
    def __init__(self, t, q, flags, ndaq=1, stride=None):
        self.t = t
        self.q = q
        self.flags = flags
        self.ndaq = ndaq
        self.stride = len(t) if stride is None else stride

    def iterate_copies(self):
        for i in range(self.ndaq):
            w = slice(i * self.stride, (i + 1) * self.stride)
            yield GPUChannels(self.t[w], self.q[w], self.flags[w])

    def get(self):
        t = self.t.get()
        q = self.q.get()
        # as in the reference: a channel whose time is still the reset value (1e9) was not hit
        return event.Channels(t < 1e8, t, q, self.flags.get())

    def __len__(self):
        return self.t.size


def _padded_cdf(cdf_x, cdf_y):
    """Device CDF tables of len(cdf_x) points each.  Detector._pdf_to_cdf yields a cdf_y that is
    one entry SHORTER than cdf_x (chroma/detector.py:109-112) and the reference then reads
    cdf_y[len(cdf_x)-1] past the end of its device array (chroma/gpu/detector.py:34-36 passes
    len(cdf_x)); here that entry exists and is 1.0, the value a CDF ends with."""
    x = np.asarray(cdf_x, dtype=np.float32)
    y = np.asarray(cdf_y, dtype=np.float32)
    if len(y) < len(x):
        y = np.concatenate([y, np.ones(len(x) - len(y), dtype=np.float32)])
    return x, y[:len(x)]


def _make_tables(daq, gpu_detector):
    """The detector's time and charge CDFs on ``daq``'s context and the chroma_daq_tables over them: ``_tables_host``,
    ``_arrays``, ``charge_unit`` and ``tables`` of ``daq`` (GPUDaq and GPUEventDaq)."""
    det = gpu_detector.geometry
    tx, ty = _padded_cdf(*det.time_cdf)
    qx, qy = _padded_cdf(*det.charge_cdf)
    daq._tables_host = (tx, ty, qx, qy)
    daq._arrays = [to_gpu(a, ctx=daq.ctx) for a in (tx, ty, qx, qy)]
    daq.charge_unit = float(np.float32(det.charge_cdf[0][-1] / 2 ** 16))
    daq.tables = _lib.DaqTables(daq._arrays[0].ptr, daq._arrays[1].ptr, len(tx),
                                daq._arrays[2].ptr, daq._arrays[3].ptr, len(qx), daq.charge_unit)


class GPUDaq(object):
    def __init__(self, gpu_detector, ndaq=1):
        if ndaq < 1:
            raise ValueError('ndaq must be at least 1')
        self.ctx = gpu_detector.ctx
        self.gpu_detector = gpu_detector
        n = gpu_detector.nchannels * ndaq
        self.earliest_time_gpu = empty(n, np.float32, self.ctx)
        self.earliest_time_int_gpu = empty(n, np.uint32, self.ctx)
        self.channel_history_gpu = zeros(n, np.uint32, self.ctx)
        self.channel_q_int_gpu = zeros(n, np.uint32, self.ctx)
        self.channel_q_gpu = zeros(n, np.float32, self.ctx)
        _make_tables(self, gpu_detector)
        self.ndaq = ndaq
        self.stride = gpu_detector.nchannels
        self.acquisition = 0

    def begin_acquire(self, nthreads_per_block=64):
        _lib.check(self.ctx._lib.chroma_daq_reset(self.ctx.handle, 1e9, len(self.earliest_time_int_gpu),
                                                  self.earliest_time_int_gpu.ptr, self.channel_q_int_gpu.ptr,
                                                  self.channel_history_gpu.ptr))
        self.channel_q_gpu.fill(0)

    def acquire(self, gpuphotons, rng_states, nthreads_per_block=64, max_blocks=1024, start_photon=None,
                nphotons=None, weight=1.0):
        if start_photon is None:
            start_photon = 0
        if nphotons is None:
            nphotons = len(gpuphotons.pos) - start_photon
        rng = gpuphotons._rng(rng_states)
        s = _structure(gpuphotons)
        if self.ndaq == 1:
            _lib.check(self.ctx._lib.chroma_daq_acquire(self.ctx.handle, self.gpu_detector.handle, ctypes.byref(self.tables),
                                                        int(start_photon), int(nphotons), event.SURFACE_DETECT,
                                                        ctypes.byref(s), rng, self.acquisition, float(weight),
                                                        self.earliest_time_int_gpu.ptr, self.channel_q_int_gpu.ptr,
                                                        self.channel_history_gpu.ptr))
        else:
            _lib.check(self.ctx._lib.chroma_daq_acquire_many(self.ctx.handle, self.gpu_detector.handle, ctypes.byref(self.tables),
                                                             int(start_photon), int(nphotons), event.SURFACE_DETECT,
                                                             ctypes.byref(s), rng, self.acquisition, float(weight),
                                                             int(self.ndaq), int(self.stride),
                                                             self.earliest_time_int_gpu.ptr, self.channel_q_int_gpu.ptr,
                                                             self.channel_history_gpu.ptr))
        self.acquisition += 1
        self.ctx.synchronize()

    def end_acquire(self, nthreads_per_block=64):
        _lib.check(self.ctx._lib.chroma_daq_convert(self.ctx.handle, len(self.earliest_time_int_gpu), self.charge_unit,
                                                    self.earliest_time_int_gpu.ptr, self.channel_q_int_gpu.ptr,
                                                    self.earliest_time_gpu.ptr, self.channel_q_gpu.ptr))
        self.ctx.synchronize()
        return GPUChannels(self.earliest_time_gpu, self.channel_q_gpu, self.channel_history_gpu, self.ndaq, self.stride)


class EventChannels(object):
    """What ``GPUEventDaq.acquire`` returns: the channels of every event of a batch, held sparse -- per chunk of events the
    touched (event, channel) words in (event, channel) order and the offsets of the events in them.  ``len()`` is the number
    of events, ``sparse(i)`` the touched channels of event i, ``[i]`` its dense ``event.Channels``."""

    def __init__(self, nchannels, nevents, rows_per_chunk, chunks):
        self.nchannels = nchannels
        self.nevents = nevents
        self.rows_per_chunk = rows_per_chunk
        self._chunks = chunks                # per chunk: (offsets, channel, t, q, flags) on the host

    def __len__(self):
        return self.nevents

    def sparse(self, i):
        """(channel ids, t, q, flags) of event ``i``: the words an accepted photon reached, in channel order, as slices of
        the chunk's arrays (no copy).  A word whose accepted times were all negative is among them with t = 1e9."""
        i = int(i)
        if i < 0:
            i += self.nevents
        if not 0 <= i < self.nevents:
            raise IndexError('event %d of %d' % (i, self.nevents))
        offsets, channel, t, q, flags = self._chunks[i // self.rows_per_chunk]
        row = i % self.rows_per_chunk
        w = slice(int(offsets[row]), int(offsets[row + 1]))
        return channel[w], t[w], q[w], flags[w]

    def __getitem__(self, i):
        """The dense ``event.Channels`` of event ``i``, bit for bit what ``GPUDaq.end_acquire().get()`` gives for it."""
        channel, ts, qs, fs = self.sparse(i)
        t = np.full(self.nchannels, 1e9, dtype=np.float32)
        q = np.zeros(self.nchannels, dtype=np.float32)
        flags = np.zeros(self.nchannels, dtype=np.uint32)
        t[channel] = ts
        q[channel] = qs
        flags[channel] = fs
        return event.Channels(t < 1e8, t, q, flags)


class GPUEventDaq(object):
    """The per-event acquisitions of a batch as one acquisition (chroma_daq_acquire_events), read back sparse
    (chroma_daq_compact_events): event r of a batch accumulates into row r of ``rows_per_chunk * nchannels`` words, as
    acquisition ``acquisition + r``, so the result is what one ``GPUDaq`` begin_acquire / acquire(start_photon, nphotons) /
    end_acquire per event gives, numbering its acquisitions on from ``acquisition``.  A batch of more events than
    ``rows_per_chunk`` is taken in chunks of that many; the result does not depend on the chunking.

    ``max_entries``: the words of each of the three accumulators.  The default, 2^24 (about 200 MB of accumulators plus
    the scan's buffers; 578 events per chunk at 29 007 channels), is a guess at a modest footprint, not a measured optimum."""

    def __init__(self, gpu_detector, max_entries=1 << 24):
        self.ctx = gpu_detector.ctx
        self.gpu_detector = gpu_detector
        self.nchannels = int(gpu_detector.nchannels)
        if self.nchannels < 1:
            raise ValueError('the detector has no channels')
        self.rows_per_chunk = max(1, int(max_entries) // self.nchannels)
        n = self.rows_per_chunk * self.nchannels
        self.earliest_time_int_gpu = empty(n, np.uint32, self.ctx)
        self.channel_q_int_gpu = empty(n, np.uint32, self.ctx)
        self.channel_history_gpu = empty(n, np.uint32, self.ctx)
        _make_tables(self, gpu_detector)
        self._offsets_gpu = None             # the compaction's outputs, grown to the largest chunk seen
        self._sparse_gpu = None

    def _compaction_buffers(self, nrows, capacity):
        if self._offsets_gpu is None or len(self._offsets_gpu) < nrows + 1:
            self._offsets_gpu = empty(nrows + 1, np.uint32, self.ctx)
        if self._sparse_gpu is None or len(self._sparse_gpu[0]) < capacity:
            self._sparse_gpu = [empty(capacity, dtype, self.ctx) for dtype in (np.int32, np.float32, np.float32, np.uint32)]
        return self._offsets_gpu, self._sparse_gpu

    def acquire(self, gpuphotons, rng_states, bounds, acquisition=0, weight=1.0):
        """One acquisition per event of ``bounds`` (len(events) + 1 ascending photon indices into ``gpuphotons``; event r is
        the photons [bounds[r], bounds[r + 1]), empty events allowed), event r as acquisition ``acquisition + r``.  Returns
        an ``EventChannels``."""
        bounds = np.asarray(bounds)
        if bounds.ndim != 1 or len(bounds) < 1 or not np.issubdtype(bounds.dtype, np.integer):
            raise ValueError('bounds: a 1-D array of at least one photon index')
        if len(bounds) and (bounds.min() < 0 or bounds.max() > 0xffffffff):
            raise ValueError('bounds: photon indices of 32 bits')
        bounds = np.ascontiguousarray(bounds, dtype=np.uint32)
        nevents = len(bounds) - 1
        rng = gpuphotons._rng(rng_states)
        s = _structure(gpuphotons)
        lib, handle, nch = self.ctx._lib, self.ctx.handle, self.nchannels
        accumulators = (self.earliest_time_int_gpu.ptr, self.channel_q_int_gpu.ptr, self.channel_history_gpu.ptr)
        chunks = []
        for first in range(0, nevents, self.rows_per_chunk):
            nrows = min(self.rows_per_chunk, nevents - first)
            b = bounds[first:first + nrows + 1]
            _lib.check(lib.chroma_daq_reset(handle, 1e9, nrows * nch, *accumulators))
            _lib.check(lib.chroma_daq_acquire_events(handle, self.gpu_detector.handle, ctypes.byref(self.tables), nrows, _lib.ptr(b),
                                                     event.SURFACE_DETECT, ctypes.byref(s), len(gpuphotons.pos), rng,
                                                     (int(acquisition) + first) & 0xffffffff, float(weight), nch, *accumulators))
            # (a touched word takes an accepted photon: never more of them than photons in the window, nor than words)
            capacity = min(int(b[-1]) - int(b[0]), nrows * nch)
            offsets, sparse = self._compaction_buffers(nrows, capacity)
            ntouched = ctypes.c_uint64(0)
            _lib.check(lib.chroma_daq_compact_events(handle, nrows, nch, nch, self.charge_unit, *accumulators, capacity,
                                                     offsets.ptr, *[a.ptr for a in sparse], ctypes.byref(ntouched)))
            chunks.append(tuple([offsets[:nrows + 1].get()] + [a[:ntouched.value].get() for a in sparse]))
        return EventChannels(nch, nevents, self.rows_per_chunk, chunks)
