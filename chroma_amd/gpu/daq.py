"""GPUDaq / GPUChannels: per-channel earliest hit time, charge and history
(reference: chroma/gpu/daq.py:8-100 over chroma/cuda/daq.cu).

``ndaq == 1`` runs ``run_daq``; ``ndaq > 1`` runs ``run_daq_many`` (daq.cu:88-150): that many
independent acquisitions of the same photons side by side, each with a unit normal jitter on the hit
time (``GPUChannels.iterate_copies`` walks them).  The random numbers a detected photon consumes
(weight gate, jitter, time smear, charge) come from Philox stream ``1 + acquisition`` of that photon
(copy i from word 8 i on), so propagation draws are not disturbed and two acquisitions of the same
photons differ.

``GPUEventDaq`` runs the per-event acquisitions of a whole batch -- what ``Simulation.simulate(run_daq=True)`` asks for -- as one
acquisition over a row of channels per event and reads the touched words back sparse (``EventChannels``).  Its
``acquire_pulses`` is the time-binned view of the same photoelectrons (chroma_daq_count_pulses / chroma_daq_acquire_pulses): per
(event, channel, time bin of a ``DaqWindow``) the number of photoelectrons, their charge, the earliest of their times and the OR
of their histories, only the bins that hold something (``EventPulses``, per event ``Pulses``).
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


class DaqWindow(object):
    """The time axis of a pulse acquisition: ``nbins`` bins of width ``dt`` from ``t0`` on (chroma_daq_window; float32 both, as
    the device bins with them).  A time is in bin ``floor((time - t0) / dt)``, evaluated in float32."""

    def __init__(self, t0, dt, nbins):
        self.t0 = float(np.float32(t0))
        self.dt = float(np.float32(dt))
        self.nbins = int(nbins)
        if not (np.isfinite(self.t0) and np.isfinite(self.dt) and self.dt > 0.0):
            raise ValueError('a DAQ window needs a finite t0 and a finite positive dt')
        if self.nbins != nbins or not 1 <= self.nbins <= 65536:
            raise ValueError('a DAQ window has 1 .. 65536 bins')

    @classmethod
    def of(cls, window):
        """``window`` itself if it is a DaqWindow, or the DaqWindow of a (t0, dt, nbins) triple."""
        if isinstance(window, cls):
            return window
        try:
            t0, dt, nbins = window
        except (TypeError, ValueError):
            raise ValueError('a DAQ window is (t0, dt, nbins)')
        return cls(t0, dt, nbins)

    def bin_edges(self):
        """The nbins + 1 nominal edges t0 + k dt (float64; the device decides a photon's bin by the float32 quotient)."""
        return self.t0 + self.dt * np.arange(self.nbins + 1, dtype=np.float64)

    def __eq__(self, other):
        return isinstance(other, DaqWindow) and (self.t0, self.dt, self.nbins) == (other.t0, other.dt, other.nbins)

    def __hash__(self):
        return hash((self.t0, self.dt, self.nbins))

    def __repr__(self):
        return 'DaqWindow(t0=%r, dt=%r, nbins=%d)' % (self.t0, self.dt, self.nbins)


class Pulses(object):
    """The pulses of ONE event (``EventPulses.event(i)``, ``ev.pulses``): per (channel, time bin) that holds an accepted photon, in
    (channel, bin) order, ``npe`` photoelectrons of charge ``q`` (``q_int`` counts of the charge unit), the earliest at
    ``t_first``, ``flags`` the OR of their histories; ``early`` and ``late``: the accepted photons before and behind the window."""

    def __init__(self, window, nchannels, channel, bin, npe, q, q_int, t_first, flags, early, late):
        self.window = window
        self.nchannels = nchannels
        self.channel, self.bin, self.npe, self.q, self.q_int, self.t_first, self.flags = channel, bin, npe, q, q_int, t_first, flags
        self.early, self.late = early, late

    def __len__(self):
        return len(self.channel)

    def bin_edges(self):
        return self.window.bin_edges()

    def waveform(self, channel):
        """(npe[nbins] uint32, q[nbins] float32) of one channel, dense."""
        channel = int(channel)
        if not 0 <= channel < self.nchannels:
            raise IndexError('channel %d of %d' % (channel, self.nchannels))
        w = slice(*np.searchsorted(self.channel, [channel, channel + 1]))
        npe = np.zeros(self.window.nbins, dtype=np.uint32)
        q = np.zeros(self.window.nbins, dtype=np.float32)
        npe[self.bin[w]] = self.npe[w]
        q[self.bin[w]] = self.q[w]
        return npe, q


class EventPulses(object):
    """What ``GPUEventDaq.acquire_pulses`` returns: the pulses of every event of a batch in (event, channel, bin) order --
    ``channel`` (int32), ``bin``, ``npe``, ``q_int``, ``flags`` (uint32) and ``t_first`` (float32), ``offsets`` (len + 1) the
    events' places in them, ``outside`` (len x 2) their early and late photons.  ``len()`` is the number of events."""

    def __init__(self, window, nchannels, charge_unit, offsets, channel, bin, npe, q_int, t_first, flags, outside):
        self.window = window
        self.nchannels = nchannels
        self.charge_unit = charge_unit
        self.offsets = offsets
        self.channel, self.bin, self.npe, self.q_int, self.t_first, self.flags = channel, bin, npe, q_int, t_first, flags
        self.q = (q_int.astype(np.float32) * np.float32(charge_unit)).astype(np.float32)          # as k_daq_convert
        self._outside = outside
        self.nevents = len(offsets) - 1

    def __len__(self):
        return self.nevents

    def bin_edges(self):
        return self.window.bin_edges()

    def _event(self, i):
        i = int(i)
        if i < 0:
            i += self.nevents
        if not 0 <= i < self.nevents:
            raise IndexError('event %d of %d' % (i, self.nevents))
        return i

    def _slice(self, i):
        i = self._event(i)
        return slice(int(self.offsets[i]), int(self.offsets[i + 1]))

    def sparse(self, i):
        """(channel, bin, npe, q, t_first, flags) of event ``i``, as slices (no copy); q = float32(q_int) * charge_unit."""
        w = self._slice(i)
        return self.channel[w], self.bin[w], self.npe[w], self.q[w], self.t_first[w], self.flags[w]

    def outside(self, i):
        """(early, late): the accepted photons of event ``i`` before t0 and behind the last bin."""
        early, late = self._outside[self._event(i)]
        return int(early), int(late)

    def event(self, i):
        """The ``Pulses`` of event ``i``: views of this object's arrays."""
        w = self._slice(i)
        early, late = self.outside(i)
        return Pulses(self.window, self.nchannels, self.channel[w], self.bin[w], self.npe[w], self.q[w], self.q_int[w], self.t_first[w],
                      self.flags[w], early, late)

    def waveform(self, i, channel):
        """(npe[nbins] uint32, q[nbins] float32) of one channel of event ``i``, dense."""
        return self.event(i).waveform(channel)


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
        self._pulse_rows_gpu = None          # acquire_pulses' outputs: per row (offsets, outside), per pulse the six arrays
        self._pulses_gpu = None

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

    def _pulse_buffers(self, nrows, capacity):
        if self._pulse_rows_gpu is None or len(self._pulse_rows_gpu[0]) < nrows + 1:
            self._pulse_rows_gpu = [empty(nrows + 1, np.uint32, self.ctx), empty(2 * nrows, np.uint32, self.ctx)]
        if self._pulses_gpu is None or len(self._pulses_gpu[0]) < capacity:
            self._pulses_gpu = [empty(capacity, dtype, self.ctx)
                                for dtype in (np.int32, np.uint32, np.uint32, np.uint32, np.float32, np.uint32)]
        return self._pulse_rows_gpu, self._pulses_gpu

    def acquire_pulses(self, gpuphotons, rng_states, bounds, window, acquisition=0, weight=1.0):
        """The time-binned view of ``acquire`` with the same arguments: the same accepted photons, per (event, channel, bin of
        ``window``: a DaqWindow or (t0, dt, nbins)).  Counts first (chroma_daq_count_pulses), then acquires into buffers grown to
        the largest count seen, ``rows_per_chunk`` events at a time.  Returns an ``EventPulses``."""
        window = DaqWindow.of(window)
        bounds = np.asarray(bounds)
        if bounds.ndim != 1 or len(bounds) < 1 or not np.issubdtype(bounds.dtype, np.integer):
            raise ValueError('bounds: a 1-D array of at least one photon index')
        if len(bounds) and (bounds.min() < 0 or bounds.max() > 0xffffffff):
            raise ValueError('bounds: photon indices of 32 bits')
        bounds = np.ascontiguousarray(bounds, dtype=np.uint32)
        nevents = len(bounds) - 1
        rng = gpuphotons._rng(rng_states)
        s = _structure(gpuphotons)
        lib, handle = self.ctx._lib, self.ctx.handle
        win = _lib.DaqWindow(window.t0, window.dt, window.nbins)
        offsets, outside = [np.zeros(1, dtype=np.int64)], []
        parts = [[] for _ in range(6)]
        total = 0
        for first in range(0, nevents, self.rows_per_chunk):
            nrows = min(self.rows_per_chunk, nevents - first)
            b = bounds[first:first + nrows + 1]
            args = (handle, self.gpu_detector.handle, ctypes.byref(self.tables), nrows, _lib.ptr(b), event.SURFACE_DETECT, ctypes.byref(s),
                    len(gpuphotons.pos), rng, (int(acquisition) + first) & 0xffffffff, float(weight), ctypes.byref(win))
            naccepted = ctypes.c_uint64(0)
            _lib.check(lib.chroma_daq_count_pulses(*(args + (ctypes.byref(naccepted),))))
            capacity = int(naccepted.value)
            (d_offsets, d_outside), arrays = self._pulse_buffers(nrows, capacity)
            npulses = ctypes.c_uint64(0)
            _lib.check(lib.chroma_daq_acquire_pulses(*(args + (capacity, d_offsets.ptr) + tuple(a.ptr for a in arrays) +
                                                       (d_outside.ptr, ctypes.byref(npulses)))))
            offsets.append(d_offsets[:nrows + 1].get()[1:].astype(np.int64) + total)
            outside.append(d_outside[:2 * nrows].get().reshape(nrows, 2))
            for part, a in zip(parts, arrays):
                part.append(a[:npulses.value].get())
            total += int(npulses.value)
        dtypes = (np.int32, np.uint32, np.uint32, np.uint32, np.float32, np.uint32)
        columns = [np.concatenate(part) if part else np.zeros(0, dtype=dtype) for part, dtype in zip(parts, dtypes)]
        outside = np.concatenate(outside) if outside else np.zeros((0, 2), dtype=np.uint32)
        return EventPulses(window, self.nchannels, self.charge_unit, np.concatenate(offsets), *columns, outside=outside)
