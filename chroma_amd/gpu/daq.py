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
of their histories, only the bins that hold something (``EventPulses``, per event ``Pulses``).  With a ``DaqTrigger`` the pulses are
triggered where they lie on the device (chroma_daq_trigger_pulses): the firings of a multiplicity or photoelectron sum over a
coincidence window, and per firing the channels of its readout gate (``EventTriggers``, per event ``Triggers``);
``EventPulses.trigger`` is the same computed in NumPy on the host arrays.  With a ``DaqNoise`` the PMTs' dark counts are drawn on
the device as further photoelectrons of the pulses (chroma_daq_acquire_pulses_noise), flagged ``event.DARK_NOISE``, and reach
the trigger like any other; ``DaqNoise.sample`` draws the same ones on the host.
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
    ``t_first``, ``flags`` the OR of their histories; ``early`` and ``late``: the accepted photons before and behind the window;
    ``noise``: the dark-noise photoelectrons among the event's (0 without a ``DaqNoise``)."""

    def __init__(self, window, nchannels, channel, bin, npe, q, q_int, t_first, flags, early, late, noise=0):
        self.window = window
        self.nchannels = nchannels
        self.channel, self.bin, self.npe, self.q, self.q_int, self.t_first, self.flags = channel, bin, npe, q, q_int, t_first, flags
        self.early, self.late = early, late
        self.noise = noise

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
    events' places in them, ``outside`` (len x 2) their early and late photons, ``noise`` (len, uint32) the dark-noise
    photoelectrons of every event (zeros without a ``DaqNoise``).  ``len()`` is the number of events."""

    def __init__(self, window, nchannels, charge_unit, offsets, channel, bin, npe, q_int, t_first, flags, outside, noise=None):
        self.window = window
        self.nchannels = nchannels
        self.charge_unit = charge_unit
        self.offsets = offsets
        self.channel, self.bin, self.npe, self.q_int, self.t_first, self.flags = channel, bin, npe, q_int, t_first, flags
        self.q = (q_int.astype(np.float32) * np.float32(charge_unit)).astype(np.float32)          # as k_daq_convert
        self._outside = outside
        self.nevents = len(offsets) - 1
        self.noise = np.zeros(self.nevents, dtype=np.uint32) if noise is None else noise
        self.triggers = None                 # the EventTriggers of acquire_pulses(trigger=...)

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
                      self.flags[w], early, late, int(self.noise[self._event(i)]))

    def waveform(self, i, channel):
        """(npe[nbins] uint32, q[nbins] float32) of one channel of event ``i``, dense."""
        return self.event(i).waveform(channel)

    def trigger(self, trigger):
        """The ``EventTriggers`` of these pulses under ``trigger`` (a DaqTrigger or its tuple), computed in NumPy on the host
        arrays -- no GPU, no library: what ``GPUEventDaq.acquire_pulses(trigger=...)`` computes on the device, bit for bit."""
        return trigger_pulses_host(self.window, trigger, self.nchannels, self.charge_unit, self.offsets, self.channel, self.bin, self.npe,
                                   self.q_int, self.t_first, self.flags)


class DaqNoise(object):
    """PMT dark noise for the pulses of a ``DaqWindow`` (chroma_daq_noise): ``rate_hz`` is one dark rate for every channel or
    one per channel, finite and not negative; all-zero rates mean no noise (``off``).  Per (event, channel) the device draws a
    Poisson number of candidates at the LARGEST rate from an integer table and keeps each with probability rate / largest
    rate; a kept one falls uniformly into the window, takes a charge from the detector's charge CDF and carries ``flag`` as
    its history (include/chroma_hip.h, "dark noise").

    ``tables`` builds the integer tables in float64.  With mu = max(rate) * 1e-9 * nbins * dt (dt in ns) the expected
    candidates per (event, channel), the count table holds floor(P(X <= j) * 2^32) up to the first entry that saturates at
    2^32 - 1, and it has 64 entries at most: that holds up to mu = 25.976 (where P(X > 63) passes 2^-32), so every mu up to
    ``MAX_MU`` = 25.9 has its table and from mu = 26 on ``tables`` raises ValueError -- take a shorter window."""

    MAX_COUNT = 64
    MAX_MU = 25.9

    def __init__(self, rate_hz, flag=event.DARK_NOISE):
        rate = np.asarray(rate_hz, dtype=np.float64)
        if rate.ndim > 1 or rate.size < 1 or not np.isfinite(rate).all() or (rate < 0).any():
            raise ValueError('dark rates: a finite rate that is not negative, or one per channel')
        self.rate_hz = rate
        self.flag = int(flag)
        if self.flag != flag or not 0 < self.flag <= 0xffffffff or self.flag & (self.flag - 1):
            raise ValueError('the flag of the noise is one history bit')
        self.off = not (rate > 0).any()

    @classmethod
    def of(cls, noise):
        """``noise`` itself if it is a DaqNoise, or the DaqNoise of a rate (or of the rates per channel)."""
        return noise if isinstance(noise, cls) else cls(noise)

    def mu(self, window):
        """The expected candidates per (event, channel): the largest rate over the whole window."""
        window = DaqWindow.of(window)
        return float(self.rate_hz.max()) * 1e-9 * window.nbins * window.dt

    def tables(self, window, nchannels):
        """(count_cdf, accept): the uint32 arrays of chroma_daq_noise for ``window`` and a detector of ``nchannels``."""
        nchannels = int(nchannels)
        if self.rate_hz.ndim == 1 and len(self.rate_hz) != nchannels:
            raise ValueError('%d dark rates for %d channels' % (len(self.rate_hz), nchannels))
        if self.off:
            raise ValueError('no channel has a dark rate: there are no tables (DaqNoise.off)')
        mu = self.mu(window)
        top = float(self.rate_hz.max())
        p = np.exp(-mu)
        total = 0.0
        cdf = []
        for j in range(self.MAX_COUNT):
            total += p
            entry = min(int(np.floor(total * 2.0 ** 32)), 2 ** 32 - 1)
            cdf.append(entry)
            if entry == 2 ** 32 - 1:
                break
            p = p * mu / (j + 1)
        else:
            raise ValueError('mu = %g candidates per channel and event: more than a table of %d entries holds (mu <= %g)' % (mu, self.MAX_COUNT, self.MAX_MU))
        accept = np.floor(np.broadcast_to(self.rate_hz, (nchannels,)) / top * 2.0 ** 31 + 0.5).astype(np.uint32)
        return np.array(cdf, dtype=np.uint32), accept

    def sample(self, window, nrows, nchannels, charge_cdf, charge_unit, seed=0, acquisition=0):
        """The kept noise photoelectrons of ``nrows`` events on the HOST (chroma_daq_noise_host: no GPU), bit for bit what
        ``GPUEventDaq.acquire_pulses(noise=self, acquisition=acquisition)`` mixes into the pulses of a context seeded with ``seed``:
        a structured array of (row, channel, bin, time, charge_int) in (row, channel, candidate) order.  ``charge_cdf``: the (x, y)
        of the detector's charge CDF as the DAQ holds it; ``charge_unit``: its charge unit."""
        window = DaqWindow.of(window)
        dtype = [('row', np.uint32), ('channel', np.uint32), ('bin', np.uint32), ('time', np.float32), ('charge_int', np.uint32)]
        if self.off:
            return np.zeros(0, dtype=dtype)
        lib = _lib.load()
        count_cdf, accept = self.tables(window, nchannels)
        qx, qy = _padded_cdf(*charge_cdf)
        qx, qy = np.ascontiguousarray(qx), np.ascontiguousarray(qy)
        tables = _lib.DaqTables(None, None, 0, _lib.ptr(qx), _lib.ptr(qy), len(qx), float(charge_unit))
        win = _lib.DaqWindow(window.t0, window.dt, window.nbins)
        struct = _lib.DaqNoise(_lib.ptr(count_cdf), len(count_cdf), _lib.ptr(accept), self.flag)
        n = ctypes.c_uint64(0)
        capacity = 0
        columns = [np.zeros(0, dtype=np.uint32) for _ in range(5)]
        for attempt in range(2):
            rc = lib.chroma_daq_noise_host(ctypes.byref(tables), ctypes.byref(win), ctypes.byref(struct), int(nrows), int(nchannels),
                                           int(seed), int(acquisition) & 0xffffffff, capacity,
                                           *([_lib.ptr(a) if capacity else None for a in columns] + [ctypes.byref(n)]))
            if rc == 0 or attempt or n.value <= capacity:
                break
            capacity = int(n.value)
            columns = [np.zeros(capacity, dtype=np.uint32) for _ in range(5)]
        _lib.check(rc)
        out = np.zeros(int(n.value), dtype=dtype)
        for (name, kind), a in zip(dtype, columns):
            out[name] = a[:len(out)].view(kind)
        return out


NO_TRIGGER = 0xffffffff          # pulse_trigger of a pulse that lies in no gate


class DaqTrigger(object):
    """A trigger on the pulses of a ``DaqWindow`` (chroma_daq_trigger; everything in BINS of the window).  The sum S(b) of a bin
    is over the pulses of the bins (b - width, b]: the number of distinct channels among them (``kind='nhit'``) or their
    photoelectrons (``'npe'``).  Through the bins ascending the trigger fires at b if S(b) >= threshold and b is not within
    ``holdoff`` bins behind the last firing; the gate of a firing is the bins [b - pre, b + post), clipped to the window.
    Defaults: ``post = width`` and ``holdoff = pre + post`` (the smallest allowed: the gates of an event never overlap)."""

    KINDS = {'nhit': 0, 'npe': 1}

    def __init__(self, threshold, width, holdoff=None, pre=0, post=None, kind='nhit'):
        if kind not in self.KINDS:
            raise ValueError("a DAQ trigger's kind is 'nhit' or 'npe'")
        self.kind = kind
        values = {}
        for name, value in (('threshold', threshold), ('width', width), ('pre', pre), ('post', width if post is None else post), ('holdoff', holdoff)):
            if name == 'holdoff' and value is None:
                value = values['pre'] + values['post']
            try:
                whole = int(value)
            except (TypeError, ValueError):
                raise ValueError('a DAQ trigger\'s %s is a whole number of bins' % name)
            if whole != value or not 0 <= whole <= 0xffffffff:
                raise ValueError('a DAQ trigger\'s %s is a whole number of 32 bits' % name)
            values[name] = whole
        values = [values[name] for name in ('threshold', 'width', 'holdoff', 'pre', 'post')]
        self.threshold, self.width, self.holdoff, self.pre, self.post = values
        if self.threshold < 1 or self.width < 1 or self.post < 1:
            raise ValueError('a DAQ trigger needs a threshold, a width and a post of at least 1')
        if self.holdoff < max(1, self.pre + self.post):
            raise ValueError('a DAQ trigger needs holdoff >= max(1, pre + post): the gates of an event do not overlap')

    @classmethod
    def of(cls, trigger):
        """``trigger`` itself if it is a DaqTrigger, or the DaqTrigger of a (threshold, width[, holdoff, pre, post[, kind]]) tuple."""
        if isinstance(trigger, cls):
            return trigger
        try:
            parts = tuple(trigger)
        except TypeError:
            raise ValueError('a DAQ trigger is (threshold, width[, holdoff, pre, post[, kind]])')
        if not 2 <= len(parts) <= 6:
            raise ValueError('a DAQ trigger is (threshold, width[, holdoff, pre, post[, kind]])')
        return cls(*parts)

    def check(self, window):
        """Raises ValueError unless the trigger fits ``window`` (a coincidence window of at most its bins)."""
        if self.width > window.nbins:
            raise ValueError('a DAQ trigger of width %d on a window of %d bins' % (self.width, window.nbins))
        return self

    def struct(self):
        return _lib.DaqTrigger(self.KINDS[self.kind], self.threshold, self.width, self.holdoff, self.pre, self.post)

    def _key(self):
        return (self.kind, self.threshold, self.width, self.holdoff, self.pre, self.post)

    def __eq__(self, other):
        return isinstance(other, DaqTrigger) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return 'DaqTrigger(threshold=%d, width=%d, holdoff=%d, pre=%d, post=%d, kind=%r)' % (
            self.threshold, self.width, self.holdoff, self.pre, self.post, self.kind)


CLIPPED_HIGH, CLIPPED_LOW = 1, 2          # the bits of a trace's flag word: some sample clipped at the top, some at 0


class DaqDigitizer(object):
    """The digitiser of a trigger's gates (chroma_daq_digitizer): every gated (firing, channel) is read out as a trace of
    ``pre + post`` ADC samples, one per bin from ``pre`` bins before the firing on.  ``shape`` is the response to one unit of the
    detector's charge, in ADC counts per bin from the pulse's own bin on (1 .. 1024 bins; it may be negative); pulses pile up, and
    pulses from before the gate have their tails in it.  ``pedestal`` (ADC counts) is added, then electronics noise -- a Gaussian
    of ``noise_sigma`` ADC counts rounded to whole counts, one draw per (event, channel, bin) whichever firing reads it -- and the
    sample is clipped to ``bits`` bits; ``trace_flags`` says where that happened (``CLIPPED_HIGH``, ``CLIPPED_LOW``).  The
    arithmetic is fixed point with ``shift`` fractional bits (include/chroma_hip.h, "digitiser").

    ``tables`` builds the integer tables in float64: tap d = round(shape[d] * charge_unit * 2^shift), the response to one charge
    COUNT, and for the noise ``noise_lo = -32`` and 64 entries floor(Phi((noise_lo + j + 0.5) / sigma) * 2^32), saturated at
    2^32 - 1 -- every sigma up to ``MAX_SIGMA`` = 8 out to 4 sigma."""

    MAX_TAPS = 1024
    MAX_NOISE = 64
    NOISE_LO = -32
    MAX_SIGMA = 8.0

    def __init__(self, shape, pedestal=0, bits=14, shift=16, noise_sigma=0.0):
        shape = np.array(shape, dtype=np.float64)
        if shape.ndim != 1 or not 1 <= len(shape) <= self.MAX_TAPS or not np.isfinite(shape).all():
            raise ValueError('a digitiser\'s shape is 1 .. %d finite values' % self.MAX_TAPS)
        shape.setflags(write=False)
        self.shape = shape
        for name, value, lo, hi in (('pedestal', pedestal, -2 ** 31, 2 ** 31 - 1), ('bits', bits, 1, 16), ('shift', shift, 0, 31)):
            try:
                whole = int(value)
            except (TypeError, ValueError):
                raise ValueError('a digitiser\'s %s is a whole number' % name)
            if whole != value or not lo <= whole <= hi:
                raise ValueError('a digitiser\'s %s is a whole number of %d .. %d' % (name, lo, hi))
            setattr(self, name, whole)
        self.noise_sigma = float(noise_sigma)
        if not 0.0 <= self.noise_sigma <= self.MAX_SIGMA:
            raise ValueError('a digitiser\'s noise has a sigma of 0 .. %g ADC counts: the table holds no more' % self.MAX_SIGMA)

    @classmethod
    def biexponential(cls, amplitude, rise_ns, fall_ns, dt, length=None, **kw):
        """The digitiser whose shape is exp(-t / fall_ns) - exp(-t / rise_ns), scaled so that the curve peaks at ``amplitude``
        ADC counts per unit charge, sampled at the centres t = (d + 0.5) dt of the bins (``dt`` in ns) from the pulse's own on.
        ``length`` bins; by default up to where the curve has fallen to a thousandth of its peak, 1024 at the most."""
        amplitude, rise, fall, dt = float(amplitude), float(rise_ns), float(fall_ns), float(dt)
        if not (0.0 < rise < fall < float('inf')) or not (0.0 < dt < float('inf')) or not np.isfinite(amplitude):
            raise ValueError('a biexponential pulse needs 0 < rise_ns < fall_ns, a positive dt and a finite amplitude')
        t_peak = np.log(fall / rise) * rise * fall / (fall - rise)
        peak = np.exp(-t_peak / fall) - np.exp(-t_peak / rise)
        if length is None:
            length = int(min(cls.MAX_TAPS, max(1, np.ceil((t_peak + fall * np.log(1000.0)) / dt))))
        if int(length) != length or not 1 <= int(length) <= cls.MAX_TAPS:
            raise ValueError('a digitiser\'s shape has 1 .. %d bins' % cls.MAX_TAPS)
        t = (np.arange(int(length), dtype=np.float64) + 0.5) * dt
        return cls(amplitude * (np.exp(-t / fall) - np.exp(-t / rise)) / peak, **kw)

    @classmethod
    def of(cls, digitizer):
        """``digitizer`` itself if it is a DaqDigitizer, or the biexponential one of an (amplitude, rise_ns, fall_ns, dt[, bits[,
        pedestal[, sigma]]]) tuple."""
        if isinstance(digitizer, cls):
            return digitizer
        try:
            parts = tuple(digitizer)
        except TypeError:
            raise ValueError('a DAQ digitiser is (amplitude, rise_ns, fall_ns, dt[, bits[, pedestal[, sigma]]])')
        if not 4 <= len(parts) <= 7:
            raise ValueError('a DAQ digitiser is (amplitude, rise_ns, fall_ns, dt[, bits[, pedestal[, sigma]]])')
        kw = dict(zip(('bits', 'pedestal', 'noise_sigma'), parts[4:]))
        try:
            return cls.biexponential(*[float(x) for x in parts[:4]], **kw)
        except TypeError:
            raise ValueError('a DAQ digitiser is (amplitude, rise_ns, fall_ns, dt[, bits[, pedestal[, sigma]]])')

    def check(self, trigger):
        """Raises ValueError unless ``trigger``'s gate is one this digitiser can read: pre + post of 65536 samples at the most."""
        if trigger.pre + trigger.post > 65536:
            raise ValueError('a gate of %d samples: a trace holds 65536' % (trigger.pre + trigger.post))
        return self

    def tables(self, charge_unit):
        """(taps int32, noise_cdf uint32 -- empty without noise --, noise_lo) of chroma_daq_digitizer for a detector whose
        charge counts are of ``charge_unit``."""
        charge_unit = float(charge_unit)
        if not (0.0 < charge_unit < float('inf')):
            raise ValueError('a charge unit is finite and positive')
        taps = np.rint(self.shape * charge_unit * 2.0 ** self.shift)
        if not np.isfinite(taps).all() or (taps > 2 ** 31 - 1).any() or (taps < -2 ** 31).any():
            raise ValueError('the taps do not fit 32 bits: a smaller shift, or a smaller shape')
        cdf = np.zeros(0, dtype=np.uint32)
        if self.noise_sigma > 0.0:
            import math
            x = (self.NOISE_LO + np.arange(self.MAX_NOISE, dtype=np.float64) + 0.5) / self.noise_sigma
            phi = np.array([0.5 * (1.0 + math.erf(v / math.sqrt(2.0))) for v in x], dtype=np.float64)
            cdf = np.minimum(np.floor(phi * 2.0 ** 32), 2.0 ** 32 - 1).astype(np.uint32)
        return taps.astype(np.int32), cdf, self.NOISE_LO

    def struct(self, charge_unit):
        """(the chroma_daq_digitizer, the host arrays it points to: keep them alive as long as it is used)"""
        taps, cdf, lo = self.tables(charge_unit)
        return _lib.DaqDigitizer(_lib.ptr(taps), len(taps), self.shift, self.pedestal, self.bits, _lib.ptr(cdf) if len(cdf) else None,
                                 len(cdf), lo), (taps, cdf)

    def _key(self):
        return (self.shape.tobytes(), self.pedestal, self.bits, self.shift, self.noise_sigma)

    def __eq__(self, other):
        return isinstance(other, DaqDigitizer) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return 'DaqDigitizer(shape=<%d bins, peak %g>, pedestal=%d, bits=%d, shift=%d, noise_sigma=%r)' % (
            len(self.shape), float(np.abs(self.shape).max()), self.pedestal, self.bits, self.shift, self.noise_sigma)


TIME_AT_EDGE, OPEN_AT_START, OPEN_AT_END = 1, 2, 4          # the bits of a found pulse's flag word
BASELINE_BUSY = 1                                           # the bit of a reduced trace's flag word
# the per-pulse arrays of a trace reduction, in the order of chroma_daq_reduce_traces' arguments
FOUND_COLUMNS = (('found_start', np.uint32), ('found_width', np.uint32), ('found_peak', np.uint32), ('found_peak_sample', np.uint32),
                 ('found_integral', np.int64), ('found_time', np.uint32), ('found_flags', np.uint32))


class DaqReducer(object):
    """The reduction of digitised traces (chroma_daq_reducer): what the electronics make of a trace -- the pulses in it, the
    charge of each and a constant-fraction time.  The baseline is the mean of the first ``nbaseline`` samples (0 .. 64), or
    ``pedestal`` when that is 0 (``BASELINE_BUSY`` when they spread by more than ``baseline_spread`` counts); a pulse is
    ``min_width`` or more consecutive samples ``threshold`` ADC counts or more above it (below, with ``polarity=-1``), integrated from
    ``lead`` samples before to ``lag`` samples behind it but never into a neighbour's window, and timed where its leading edge
    crosses the fraction ``cfd`` (1/256 .. 1) of its peak, interpolated to 1/256 of a sample.  The arithmetic is integer
    (include/chroma_hip.h, "trace reduction").

    ``time_offset_ns`` is subtracted from the times ``Triggers.found`` and ``reco`` give (the shape's rise to the fraction);
    ``gain``, ADC counts x bins per unit of the detector's charge (``for_digitizer``: the sum of the shape), turns integrals into
    charges."""

    def __init__(self, threshold, polarity=1, nbaseline=0, pedestal=0, baseline_spread=0, min_width=1, lead=0, lag=0, cfd=0.5, time_offset_ns=0.0,
                 gain=None):
        ranges = (('threshold', threshold, 1, 65535), ('polarity', polarity, -1, 1), ('nbaseline', nbaseline, 0, 64), ('pedestal', pedestal, 0, 65535),
                  ('baseline_spread', baseline_spread, 0, 0xffffffff), ('min_width', min_width, 1, 65536), ('lead', lead, 0, 65535), ('lag', lag, 0, 65535))
        for name, value, lo, hi in ranges:
            try:
                whole = int(value)
            except (TypeError, ValueError):
                raise ValueError('a reducer\'s %s is a whole number' % name)
            if whole != value or not lo <= whole <= hi or (name == 'polarity' and whole == 0):
                raise ValueError('a reducer\'s %s is a whole number of %d .. %d%s' % (name, lo, hi, ', not 0' if name == 'polarity' else ''))
            setattr(self, name, whole)
        try:
            fraction = float(cfd)
        except (TypeError, ValueError):
            raise ValueError('a reducer\'s constant fraction is a number')
        if not (fraction == fraction) or not 1 <= int(round(fraction * 256)) <= 256:
            raise ValueError('a reducer\'s constant fraction is 1/256 .. 1')
        self.cfd = int(round(fraction * 256))          # in 1/256
        self.time_offset_ns = float(time_offset_ns)
        self.gain = None if gain is None else float(gain)
        if not np.isfinite(self.time_offset_ns) or (self.gain is not None and not (np.isfinite(self.gain) and self.gain != 0.0)):
            raise ValueError('a reducer\'s time offset is finite, its gain finite and not 0')

    @classmethod
    def for_digitizer(cls, digitizer, threshold, **kw):
        """The reducer that fits ``digitizer``'s traces: the polarity of its shape's largest excursion, its pedestal, and
        ``gain = sum(shape)``, ADC counts x bins per unit charge."""
        shape = digitizer.shape
        kw.setdefault('polarity', 1 if shape[int(np.argmax(np.abs(shape)))] >= 0.0 else -1)
        kw.setdefault('pedestal', digitizer.pedestal)
        gain = float(shape.sum())
        kw.setdefault('gain', gain if gain != 0.0 else None)
        return cls(threshold, **kw)

    @classmethod
    def of(cls, reducer):
        """``reducer`` itself if it is a DaqReducer, or the one of a (threshold[, lead, lag[, cfd[, nbaseline[, min_width]]]]) tuple."""
        if isinstance(reducer, cls):
            return reducer
        try:
            parts = tuple(reducer)
        except TypeError:
            raise ValueError('a DAQ reducer is (threshold[, lead, lag[, cfd[, nbaseline[, min_width]]]])')
        if len(parts) not in (1, 3, 4, 5, 6):
            raise ValueError('a DAQ reducer is (threshold[, lead, lag[, cfd[, nbaseline[, min_width]]]])')
        return cls(parts[0], **dict(zip(('lead', 'lag', 'cfd', 'nbaseline', 'min_width'), parts[1:])))

    def check(self, G):
        """Raises ValueError unless traces of ``G`` samples can be reduced: 1 .. 65536 of them, the baseline's at least."""
        if not 1 <= G <= 65536 or self.nbaseline > G:
            raise ValueError('a reducer with a baseline of %d samples on traces of %d: traces have 1 .. 65536 samples, the baseline\'s at least' % (self.nbaseline, G))
        return self

    @property
    def N(self):
        """What ``found_integral`` and ``found_peak`` are scaled by: max(nbaseline, 1)."""
        return max(self.nbaseline, 1)

    def struct(self):
        return _lib.DaqReducer(self.polarity, self.nbaseline, self.pedestal, self.baseline_spread, self.threshold, self.min_width, self.lead, self.lag, self.cfd)

    def _key(self):
        return (self.threshold, self.polarity, self.nbaseline, self.pedestal, self.baseline_spread, self.min_width, self.lead, self.lag, self.cfd,
                self.time_offset_ns, self.gain)

    def __eq__(self, other):
        return isinstance(other, DaqReducer) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return ('DaqReducer(threshold=%d, polarity=%d, nbaseline=%d, pedestal=%d, baseline_spread=%d, min_width=%d, lead=%d, lag=%d, cfd=%d/256, '
                'time_offset_ns=%r, gain=%r)' % (self.threshold, self.polarity, self.nbaseline, self.pedestal, self.baseline_spread, self.min_width,
                                                self.lead, self.lag, self.cfd, self.time_offset_ns, self.gain))


def reduce_traces_host(adc, reducer):
    """chroma_daq_reduce_host (no GPU) on ``adc`` (traces x samples, uint16) under ``reducer``: (found_offsets int64 (traces + 1),
    trace_base int32, reduced_flags uint32, then the arrays of ``FOUND_COLUMNS``).  Called twice: the first call counts."""
    adc = np.ascontiguousarray(adc, dtype=np.uint16)
    if adc.ndim != 2:
        raise ValueError('traces are a (traces, samples) array')
    ntraces, G = adc.shape
    reducer = DaqReducer.of(reducer).check(G)
    lib = _lib.load()
    struct = reducer.struct()
    offsets, base, flags = np.zeros(ntraces + 1, dtype=np.uint32), np.zeros(ntraces, dtype=np.int32), np.zeros(ntraces, dtype=np.uint32)
    nfound = ctypes.c_uint64(0)
    columns = [np.zeros(0, dtype=kind) for _, kind in FOUND_COLUMNS]
    for attempt in range(2):
        capacity = len(columns[0])
        rc = lib.chroma_daq_reduce_host(ctypes.byref(struct), G, ntraces, _lib.ptr(adc), capacity, _lib.ptr(offsets), _lib.ptr(base), _lib.ptr(flags),
                                        *([_lib.ptr(a) if capacity else None for a in columns] + [ctypes.byref(nfound)]))
        if rc == 0 or attempt or nfound.value <= capacity:
            break
        columns = [np.zeros(int(nfound.value), dtype=kind) for _, kind in FOUND_COLUMNS]
    _lib.check(rc)
    return [offsets.astype(np.int64), base, flags] + [a[:int(nfound.value)] for a in columns]


def _set_found(self, found):
    """The attributes of a trace reduction on a ``Triggers`` or an ``EventTriggers``: ``found`` is (reducer, found_offsets,
    trace_base, reduced_flags, the arrays of FOUND_COLUMNS) or None."""
    self.reducer = self.found_offsets = self.trace_base = self.reduced_flags = None
    for name, _ in FOUND_COLUMNS:
        setattr(self, name, None)
    if found is None:
        return
    self.reducer, self.found_offsets, self.trace_base, self.reduced_flags = found[:4]
    for (name, _), a in zip(FOUND_COLUMNS, found[4]):
        setattr(self, name, a)


def _slice_found(self, h):
    """``found`` of the hits ``h`` (a slice), the offsets rebased to 0"""
    if self.reducer is None:
        return None
    f = slice(int(self.found_offsets[h.start]), int(self.found_offsets[h.stop]))
    return (self.reducer, self.found_offsets[h.start:h.stop + 1] - self.found_offsets[h.start], self.trace_base[h], self.reduced_flags[h],
            [getattr(self, name)[f] for name, _ in FOUND_COLUMNS])


class FoundPulses(object):
    """The pulses found in ONE trace (``Triggers.found``): the arrays of ``FOUND_COLUMNS`` without their prefix (``start``,
    ``width``, ``peak``, ``peak_sample``, ``integral``, ``time``, ``flags``), ``t`` (ns, float64) and ``q`` (float64: the detector's
    charge units where the reducer knows a gain, else ADC counts x samples)."""

    def __init__(self, columns, t, q):
        for (name, _), a in zip(FOUND_COLUMNS, columns):
            setattr(self, name[len('found_'):], a)
        self.t, self.q = t, q

    def __len__(self):
        return len(self.t)


class Triggers(object):
    """The triggers of ONE event (``EventTriggers.event(i)``, ``ev.triggers``): ``bin`` and ``sum`` of every firing, ascending;
    ``sparse(k)`` the channels in the gate of firing k, ``channels(k)`` the same as a dense ``event.Channels``; ``pulse_trigger``:
    per pulse of the event's ``Pulses`` the firing (numbered within the event) whose gate holds it, or ``NO_TRIGGER``.  With a
    ``DaqDigitizer`` also ``adc(k)``, ``trace(k, channel)`` and ``sample_times(k)``: the ADC traces of firing k's channels, and
    ``traces`` (hits x samples, uint16) and ``trace_flags``, a word per hit (``CLIPPED_HIGH``, ``CLIPPED_LOW``); None without one,
    as is ``digitizer``.  With a ``DaqReducer`` also ``found(k, channel)``, ``reco(k)`` and ``reco_channels(k)``: the pulses found in the
    traces, and ``found_offsets`` (hits + 1), the ``found_*`` arrays of ``FOUND_COLUMNS``, ``trace_base``, ``reduced_flags`` and ``reducer``."""

    def __init__(self, window, trigger, nchannels, charge_unit, bin, sum, hit_offsets, hit_channel, hit_npe, hit_q_int, hit_t_first,
                 hit_flags, pulse_trigger, adc=None, trace_flags=None, digitizer=None, found=None):
        self.window, self.trigger, self.nchannels, self.charge_unit = window, trigger, nchannels, charge_unit
        self.bin, self.sum = bin, sum
        _set_found(self, found)
        self.hit_offsets = hit_offsets          # (len + 1, into the hit arrays; the first is 0)
        self.hit_channel, self.hit_npe, self.hit_q_int, self.hit_t_first, self.hit_flags = hit_channel, hit_npe, hit_q_int, hit_t_first, hit_flags
        self.hit_q = (hit_q_int.astype(np.float32) * np.float32(charge_unit)).astype(np.float32)          # as k_daq_convert
        self.pulse_trigger = pulse_trigger
        self.traces, self.trace_flags, self.digitizer = adc, trace_flags, digitizer          # (hits x samples, uint16; hits, uint32)

    def __len__(self):
        return len(self.bin)

    def adc(self, k):
        """(channel, traces) of firing ``k``: the channels read out, ascending, and their traces (len(channel) x (pre + post),
        uint16), as slices (no copy)."""
        if self.traces is None:
            raise ValueError('these triggers were not digitised (daq_digitizer / digitizer=...)')
        w = self._slice(k)
        return self.hit_channel[w], self.traces[w]

    def trace(self, k, channel):
        """The trace of ``channel`` in firing ``k``; KeyError for a channel without a pulse in the gate: it was not read out."""
        channels, traces = self.adc(k)
        channel = int(channel)
        if not 0 <= channel < self.nchannels:
            raise IndexError('channel %d of %d' % (channel, self.nchannels))
        at = int(np.searchsorted(channels, channel))
        if at == len(channels) or channels[at] != channel:
            raise KeyError('channel %d has no pulse in the gate of firing %d' % (channel, k))
        return traces[at]

    def sample_times(self, k):
        """The nominal lower edges t0 + (bin - pre + s) dt of the samples of firing ``k``'s traces (float64)."""
        self._slice(k)
        first = int(self.bin[k]) - self.trigger.pre
        return self.window.t0 + self.window.dt * (first + np.arange(self.trigger.pre + self.trigger.post, dtype=np.float64))

    def _found_of(self, w):
        """the slice of the found pulses of the hits ``w``"""
        if self.reducer is None:
            raise ValueError('these triggers were not reduced (daq_reducer / reducer=... / reduce)')
        return slice(int(self.found_offsets[w.start]), int(self.found_offsets[w.stop]))

    def _found_times(self, k, time):
        """t0 + dt * (bin[k] - pre + time / 256) - time_offset_ns, as ``sample_times`` counts the samples (float64)"""
        first = int(self.bin[k]) - self.trigger.pre
        return self.window.t0 + self.window.dt * (first + time.astype(np.float64) / 256.0) - self.reducer.time_offset_ns

    def _found_charges(self, integral):
        """integral / (N * gain) where the reducer knows a gain (the detector's charge units); integral / N otherwise"""
        r = self.reducer
        scale = float(r.N) * (r.polarity * r.gain if r.gain is not None else 1.0)
        return integral.astype(np.float64) / scale

    def found(self, k, channel):
        """The ``FoundPulses`` of ``channel``'s trace in firing ``k``; KeyError for a channel that was not read out."""
        w = self._slice(k)
        channel = int(channel)
        if not 0 <= channel < self.nchannels:
            raise IndexError('channel %d of %d' % (channel, self.nchannels))
        channels = self.hit_channel[w]
        at = int(np.searchsorted(channels, channel))
        if at == len(channels) or channels[at] != channel:
            raise KeyError('channel %d has no pulse in the gate of firing %d' % (channel, k))
        f = self._found_of(slice(w.start + at, w.start + at + 1))
        columns = [getattr(self, name)[f] for name, _ in FOUND_COLUMNS]
        return FoundPulses(columns, self._found_times(k, self.found_time[f]), self._found_charges(self.found_integral[f]))

    def reco(self, k):
        """(channel, t, q, npulses, flags) of the channels of firing ``k`` with at least one found pulse, in channel order: the
        time of the trace's first found pulse (ns, float64), the charge summed over its pulses (float64, as ``FoundPulses.q``), their
        number and the OR of their flags."""
        w = self._slice(k)
        f = self._found_of(w)
        counts = np.diff(self.found_offsets[w.start:w.stop + 1])
        has = counts > 0
        first = (self.found_offsets[w.start:w.stop] - f.start)[has]
        time, integral, flags = self.found_time[f], self.found_integral[f], self.found_flags[f]
        if len(first):
            t = self._found_times(k, time[first])
            q = self._found_charges(np.add.reduceat(integral, first))
            fl = np.bitwise_or.reduceat(flags, first)
        else:
            t, q, fl = np.zeros(0, dtype=np.float64), np.zeros(0, dtype=np.float64), np.zeros(0, dtype=np.uint32)
        return self.hit_channel[w][has], t, q, counts[has].astype(np.uint32), fl.astype(np.uint32)

    def reco_channels(self, k):
        """The dense ``event.Channels`` of what was FOUND in the traces of firing ``k``: the reconstructed counterpart of
        ``channels(k)`` (t = 1e9 and not hit where no pulse was found), ready for ``Likelihood.set_event``."""
        channel, ts, qs, _, fs = self.reco(k)
        t = np.full(self.nchannels, 1e9, dtype=np.float32)
        q = np.zeros(self.nchannels, dtype=np.float32)
        flags = np.zeros(self.nchannels, dtype=np.uint32)
        t[channel] = ts
        q[channel] = qs
        flags[channel] = fs
        return event.Channels(t < 1e8, t, q, flags)

    @property
    def time(self):
        """The nominal lower edge t0 + bin dt of every firing's bin (float64)."""
        return self.window.t0 + self.window.dt * self.bin.astype(np.float64)

    def _slice(self, k):
        k = int(k)
        if k < 0:
            k += len(self)
        if not 0 <= k < len(self):
            raise IndexError('trigger %d of %d' % (k, len(self)))
        return slice(int(self.hit_offsets[k]), int(self.hit_offsets[k + 1]))

    def sparse(self, k):
        """(channel, npe, q, t_first, flags) of the gate of firing ``k``, in channel order, as slices (no copy)."""
        w = self._slice(k)
        return self.hit_channel[w], self.hit_npe[w], self.hit_q[w], self.hit_t_first[w], self.hit_flags[w]

    def channels(self, k):
        """The dense ``event.Channels`` of the gate of firing ``k``: a channel's earliest time and charge in the gate, built as
        ``EventChannels.__getitem__`` builds an event's (t = 1e9 and not hit where the gate holds nothing of the channel)."""
        channel, npe, qs, ts, fs = self.sparse(k)
        t = np.full(self.nchannels, 1e9, dtype=np.float32)
        q = np.zeros(self.nchannels, dtype=np.float32)
        flags = np.zeros(self.nchannels, dtype=np.uint32)
        t[channel] = ts
        q[channel] = qs
        flags[channel] = fs
        return event.Channels(t < 1e8, t, q, flags)


class EventTriggers(object):
    """The triggers of every event of a batch (``EventPulses.triggers`` after ``GPUEventDaq.acquire_pulses(trigger=...)``, or
    ``EventPulses.trigger(...)``): firings in (event, bin) order -- ``bin``, ``sum`` (uint32), ``offsets`` (len + 1) the events'
    places in them; gated hits in (firing, channel) order -- ``hit_channel`` (int32), ``hit_npe``, ``hit_q_int``, ``hit_flags``
    (uint32), ``hit_t_first`` (float32), ``hit_offsets`` (firings + 1); ``pulse_trigger`` (uint32, per pulse of the batch): the
    firing, numbered within the batch, whose gate holds the pulse, or ``NO_TRIGGER``.  Digitised (``acquire_pulses(digitizer=...)``
    or ``digitize``): ``adc`` (hits x (pre + post), uint16), the ADC trace of every gated hit, ``trace_flags`` (hits, uint32) and
    ``digitizer``; None otherwise.  ``pulses``: the (channel, bin, q_int) columns of the batch's pulses, which ``digitize`` reads.
    Reduced (``acquire_pulses(reducer=...)`` or ``reduce``): ``found_offsets`` (hits + 1, int64), the places of the traces' found pulses
    in ``found_start``, ``found_width``, ``found_peak``, ``found_peak_sample`` (uint32), ``found_integral`` (int64), ``found_time`` (1/256 of a
    sample) and ``found_flags`` (``TIME_AT_EDGE``, ``OPEN_AT_START``, ``OPEN_AT_END``); per trace ``trace_base`` (int32) and
    ``reduced_flags`` (``BASELINE_BUSY``); ``reducer``.  None otherwise."""

    def __init__(self, window, trigger, nchannels, charge_unit, pulse_offsets, offsets, bin, sum, hit_offsets, hit_channel, hit_npe,
                 hit_q_int, hit_t_first, hit_flags, pulse_trigger, adc=None, trace_flags=None, digitizer=None, pulses=None, found=None):
        self.window, self.trigger, self.nchannels, self.charge_unit = window, trigger, nchannels, charge_unit
        _set_found(self, found)
        self.pulse_offsets, self.offsets, self.bin, self.sum, self.hit_offsets = pulse_offsets, offsets, bin, sum, hit_offsets
        self.hit_channel, self.hit_npe, self.hit_q_int, self.hit_t_first, self.hit_flags = hit_channel, hit_npe, hit_q_int, hit_t_first, hit_flags
        self.pulse_trigger = pulse_trigger
        self.adc, self.trace_flags, self.digitizer = adc, trace_flags, digitizer
        self.pulses = pulses
        self.nevents = len(offsets) - 1

    def digitize(self, digitizer, seed=0, acquisition=0):
        """These triggers with the traces of their gated hits under ``digitizer``, computed on the HOST (chroma_daq_digitize_host: no
        GPU) from the pulses and triggers held here -- bit for bit what ``GPUEventDaq.acquire_pulses(trigger=..., digitizer=digitizer,
        acquisition=acquisition)`` reads back on a context seeded with ``seed``.  Event i is acquisition ``acquisition + i``.  Returns
        a new ``EventTriggers`` over the same arrays."""
        digitizer = DaqDigitizer.of(digitizer).check(self.trigger)
        if self.pulses is None:
            raise ValueError('these triggers do not hold their pulses')
        lib = _lib.load()
        struct, keep = digitizer.struct(self.charge_unit)
        win = _lib.DaqWindow(self.window.t0, self.window.dt, self.window.nbins)
        trig = self.trigger.struct()
        G = self.trigger.pre + self.trigger.post
        nhits = len(self.hit_channel)
        adc = np.zeros((nhits, G), dtype=np.uint16)
        trace_flags = np.zeros(nhits, dtype=np.uint32)
        channel, bin, q_int = [np.ascontiguousarray(a, dtype=kind) for a, kind in zip(self.pulses, (np.int32, np.uint32, np.uint32))]
        u32 = lambda a: np.ascontiguousarray(a, dtype=np.uint32)
        rows_at_once = max(1, (2 ** 31 - 1) // self.window.nbins)
        for first in range(0, self.nevents, rows_at_once):
            last = min(self.nevents, first + rows_at_once)
            p0, p1 = int(self.pulse_offsets[first]), int(self.pulse_offsets[last])
            t0, t1 = int(self.offsets[first]), int(self.offsets[last])
            h0, h1 = int(self.hit_offsets[t0]), int(self.hit_offsets[t1])
            if h1 == h0:
                continue
            offsets, trig_offsets, hit_offsets = u32(self.pulse_offsets[first:last + 1] - p0), u32(self.offsets[first:last + 1] - t0), u32(self.hit_offsets[t0:t1 + 1] - h0)
            trig_bin, hit_channel = u32(self.bin[t0:t1]), np.ascontiguousarray(self.hit_channel[h0:h1], dtype=np.int32)
            part, part_flags = adc[h0:h1], trace_flags[h0:h1]
            _lib.check(lib.chroma_daq_digitize_host(last - first, self.nchannels, ctypes.byref(win), ctypes.byref(trig), ctypes.byref(struct), int(seed),
                                                    (int(acquisition) + first) & 0xffffffff, _lib.ptr(offsets), _lib.ptr(channel[p0:p1]), _lib.ptr(bin[p0:p1]),
                                                    _lib.ptr(q_int[p0:p1]), p1 - p0, _lib.ptr(trig_offsets), _lib.ptr(trig_bin), t1 - t0, _lib.ptr(hit_offsets),
                                                    _lib.ptr(hit_channel), h1 - h0, 0, h1 - h0, part.size, _lib.ptr(part), _lib.ptr(part_flags)))
        del keep
        return EventTriggers(self.window, self.trigger, self.nchannels, self.charge_unit, self.pulse_offsets, self.offsets, self.bin, self.sum,
                             self.hit_offsets, self.hit_channel, self.hit_npe, self.hit_q_int, self.hit_t_first, self.hit_flags, self.pulse_trigger,
                             adc=adc, trace_flags=trace_flags, digitizer=digitizer, pulses=self.pulses)

    def reduce(self, reducer):
        """These triggers with the pulses found in their traces under ``reducer``, computed on the HOST (chroma_daq_reduce_host: no
        GPU) from the ``adc`` held here -- bit for bit what ``GPUEventDaq.acquire_pulses(..., reducer=reducer)`` reads back.  Returns
        a new ``EventTriggers`` over the same arrays."""
        if self.adc is None:
            raise ValueError('these triggers hold no traces (daq_digitizer / digitizer=... with keep_traces, or digitize)')
        reducer = DaqReducer.of(reducer)
        got = reduce_traces_host(self.adc, reducer)
        return EventTriggers(self.window, self.trigger, self.nchannels, self.charge_unit, self.pulse_offsets, self.offsets, self.bin, self.sum,
                             self.hit_offsets, self.hit_channel, self.hit_npe, self.hit_q_int, self.hit_t_first, self.hit_flags, self.pulse_trigger,
                             adc=self.adc, trace_flags=self.trace_flags, digitizer=self.digitizer, pulses=self.pulses,
                             found=(reducer, got[0], got[1], got[2], got[3:]))

    def __len__(self):
        return self.nevents

    def event(self, i):
        """The ``Triggers`` of event ``i``."""
        i = int(i)
        if i < 0:
            i += self.nevents
        if not 0 <= i < self.nevents:
            raise IndexError('event %d of %d' % (i, self.nevents))
        a, b = int(self.offsets[i]), int(self.offsets[i + 1])
        h = slice(int(self.hit_offsets[a]), int(self.hit_offsets[b]))
        of = self.pulse_trigger[int(self.pulse_offsets[i]):int(self.pulse_offsets[i + 1])]
        of = np.where(of == NO_TRIGGER, of, of - np.uint32(a)).astype(np.uint32)
        return Triggers(self.window, self.trigger, self.nchannels, self.charge_unit, self.bin[a:b], self.sum[a:b],
                        self.hit_offsets[a:b + 1] - self.hit_offsets[a], self.hit_channel[h], self.hit_npe[h], self.hit_q_int[h],
                        self.hit_t_first[h], self.hit_flags[h], of, adc=None if self.adc is None else self.adc[h],
                        trace_flags=None if self.trace_flags is None else self.trace_flags[h], digitizer=self.digitizer,
                        found=_slice_found(self, h))


def _time_image(bits):
    """The order-preserving image of float32 bits (daq_time_image: -0 below +0) ..."""
    return np.where(bits & np.uint32(0x80000000), ~bits, bits | np.uint32(0x80000000)).astype(np.uint32)


def _time_bits(image):
    """... and back."""
    return np.where(image & np.uint32(0x80000000), image & np.uint32(0x7fffffff), ~image).astype(np.uint32)


def _follow(first, successor):
    """The members of the chains that begin at ``first`` and go on by ``successor`` (an index, or len(successor) for none),
    ascending: pointer doubling, so a chain of k members takes log2(k) rounds."""
    m = len(successor)
    jump = np.append(successor, m)
    mark = np.zeros(m + 1, dtype=bool)
    mark[first] = True
    while True:
        reached = jump[np.flatnonzero(mark[:m])]
        reached = reached[~mark[reached] & (reached < m)]
        if len(reached) == 0:
            return np.flatnonzero(mark[:m])
        mark[reached] = True
        jump = jump[jump]


def trigger_pulses_host(window, trigger, nchannels, charge_unit, offsets, channel, bin, npe, q_int, t_first, flags):
    """chroma_daq_trigger_pulses in NumPy, on pulses in (event, channel, bin) order (``offsets`` from 0 to their number): the
    differences of the sum per (event, bin) -- a channel's overlapping coincidence intervals united by a look at the entry before --
    summed along the bins for some 2^22 (event, bin) words at a time; the firings followed from each event's first bin at or
    above threshold to the next one ``holdoff`` or more behind; every pulse looked up among its event's firings; the gated
    pulses reduced per (firing, channel) behind a stable sort.  Returns an ``EventTriggers``."""
    nbins, nch = window.nbins, int(nchannels)
    trigger = DaqTrigger.of(trigger).check(window)
    offsets = np.asarray(offsets, dtype=np.int64)
    nrows, n = len(offsets) - 1, len(channel)
    width, holdoff, pre, post = trigger.width, min(trigger.holdoff, nbins), min(trigger.pre, nbins), min(trigger.post, nbins)
    row = np.repeat(np.arange(nrows, dtype=np.int64), np.diff(offsets))
    b, ch = bin.astype(np.int64), channel.astype(np.int64)
    valid = (b < nbins) & (ch >= 0) & (ch < nch)
    up = b.copy()
    if trigger.kind == 'npe':
        amount = npe.astype(np.float64)
    else:
        amount = np.ones(n, dtype=np.float64)
        if n > 1:
            same = valid[1:] & valid[:-1] & (row[1:] == row[:-1]) & (ch[1:] == ch[:-1])
            up[1:] = np.where(same, np.maximum(b[1:], b[:-1] + width), b[1:])
    down = b + width
    counts = valid & (up < down)
    # the bins at or above threshold, in (event, bin) order
    at_row, at_bin, at_sum = [np.zeros(0, dtype=np.int64)], [np.zeros(0, dtype=np.int64)], [np.zeros(0, dtype=np.int64)]
    rows_at_once = max(1, (1 << 22) // nbins)
    for first in range(0, nrows, rows_at_once):
        k = min(rows_at_once, nrows - first)
        w = slice(int(offsets[first]), int(offsets[first + k]))
        m = counts[w]
        base = (row[w][m] - first) * nbins
        u, d, a = up[w][m], down[w][m], amount[w][m]
        total = np.bincount((base + u)[u < nbins], weights=a[u < nbins], minlength=k * nbins)
        total -= np.bincount((base + d)[d < nbins], weights=a[d < nbins], minlength=k * nbins)
        s = np.cumsum(np.rint(total).astype(np.int64).reshape(k, nbins), axis=1) & 0xffffffff
        r, c = np.nonzero(s >= trigger.threshold)
        at_row.append(r + first)
        at_bin.append(c)
        at_sum.append(s[r, c])
    at_row, at_bin, at_sum = np.concatenate(at_row), np.concatenate(at_bin), np.concatenate(at_sum)
    # the firings: the first such bin of an event, then from each the first one `holdoff` or more bins behind it
    key = at_row * (2 * nbins) + at_bin
    successor = np.searchsorted(key, key + holdoff)
    inside = successor < len(key)
    inside[inside] = at_row[successor[inside]] == at_row[inside]
    successor = np.where(inside, successor, len(key))
    starts = np.flatnonzero(np.concatenate(([True], at_row[1:] != at_row[:-1]))) if len(key) else np.zeros(0, dtype=np.int64)
    fired = _follow(starts, successor)
    t_row, t_bin, t_sum = at_row[fired], at_bin[fired], at_sum[fired]
    ntriggers = len(fired)
    trig_offsets = np.searchsorted(t_row, np.arange(nrows + 1))
    # the gate of every pulse: the last firing of its event at or before bin + pre, if the pulse is before its bin + post
    found = np.searchsorted(t_row * (4 * nbins) + t_bin, row * (4 * nbins) + b + pre, side='right') - 1
    gated = valid & (found >= 0)
    at = found[gated]
    gated[gated] = (t_row[at] == row[gated]) & (b[gated] < t_bin[at] + post)
    pulse_trigger = np.where(gated, found, NO_TRIGGER).astype(np.uint32)
    # the hits: the gated pulses per (firing, channel)
    source = np.flatnonzero(gated)
    hit_key = found[source] * nch + ch[source]
    order = np.argsort(hit_key, kind='stable')
    hit_key, source = hit_key[order], source[order]
    if len(source):
        heads = np.flatnonzero(np.concatenate(([True], hit_key[1:] != hit_key[:-1])))
        hit_npe = np.add.reduceat(npe[source].astype(np.uint32), heads)
        hit_q = np.add.reduceat(q_int[source].astype(np.uint32), heads)          # (wrapping)
        hit_t = _time_bits(np.minimum.reduceat(_time_image(np.ascontiguousarray(t_first[source], dtype=np.float32).view(np.uint32)), heads))
        hit_flags = np.bitwise_or.reduceat(flags[source].astype(np.uint32), heads)
        hit_key = hit_key[heads]
    else:
        hit_npe = hit_q = hit_t = hit_flags = np.zeros(0, dtype=np.uint32)
    hit_offsets = np.searchsorted(hit_key // nch, np.arange(ntriggers + 1))
    return EventTriggers(window, trigger, nch, charge_unit, offsets, trig_offsets.astype(np.int64), t_bin.astype(np.uint32),
                         t_sum.astype(np.uint32), hit_offsets.astype(np.int64), (hit_key % nch).astype(np.int32), hit_npe.astype(np.uint32),
                         hit_q.astype(np.uint32), hit_t.view(np.float32), hit_flags.astype(np.uint32), pulse_trigger, pulses=(channel, bin, q_int))


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
        self.max_entries = max(1, int(max_entries))
        self.rows_per_chunk = max(1, self.max_entries // self.nchannels)
        n = self.rows_per_chunk * self.nchannels
        self.earliest_time_int_gpu = empty(n, np.uint32, self.ctx)
        self.channel_q_int_gpu = empty(n, np.uint32, self.ctx)
        self.channel_history_gpu = empty(n, np.uint32, self.ctx)
        _make_tables(self, gpu_detector)
        self._offsets_gpu = None             # the compaction's outputs, grown to the largest chunk seen
        self._sparse_gpu = None
        self._pulse_rows_gpu = None          # acquire_pulses' outputs: per row (offsets, outside), per pulse the six arrays
        self._pulses_gpu = None
        self._noise_tables = None            # acquire_pulses(noise=...): ((noise, window), the chroma_daq_noise, its arrays), the last one
        self._trigger_rows_gpu = None        # acquire_pulses(trigger=...): per row the offsets; per trigger (bin, sum, hit offsets) in one
        self._triggers_gpu = None            # buffer; per hit the five arrays and per pulse its trigger in another
        self._trigger_hits_gpu = None
        self._trigger_device = None          # what the last _trigger_chunk left on the device, for the digitiser
        self._adc_gpu = None                 # acquire_pulses(digitizer=...): the samples of one slice of hits ...
        self._trace_flags_gpu = None         # ... and its flag words, each grown on its own (a shorter gate: fewer samples, more traces)
        self._found_rows_gpu = None          # acquire_pulses(reducer=...): per trace of a slice (offsets + 1, base, flags) in one buffer ...
        self._found_gpu = None               # ... and per found pulse the arrays of FOUND_COLUMNS, grown to what a call reports

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
            self._pulse_rows_gpu = [empty(nrows + 1, np.uint32, self.ctx), empty(2 * nrows, np.uint32, self.ctx), empty(nrows, np.uint32, self.ctx)]
        if self._pulses_gpu is None or len(self._pulses_gpu[0]) < capacity:
            self._pulses_gpu = [empty(capacity, dtype, self.ctx)
                                for dtype in (np.int32, np.uint32, np.uint32, np.uint32, np.float32, np.uint32)]
        return self._pulse_rows_gpu, self._pulses_gpu

    def _noise_struct(self, noise, window):
        """The chroma_daq_noise of ``noise`` under ``window`` on this context: built and uploaded once per (noise, window)."""
        key = (noise, window)
        if self._noise_tables is None or self._noise_tables[0] != key:
            count_cdf, accept = noise.tables(window, self.nchannels)
            d_accept = to_gpu(accept, ctx=self.ctx)
            self._noise_tables = (key, _lib.DaqNoise(_lib.ptr(count_cdf), len(count_cdf), d_accept.ptr, noise.flag), (count_cdf, d_accept))
        return self._noise_tables[1]

    def _trigger_chunk(self, win, trigger, nrows, d_offsets, arrays, npulses):
        """chroma_daq_trigger_pulses on the pulses of one chunk where acquire_pulses left them; the host arrays (offsets, bin, sum,
        hit offsets, the five hit arrays, pulse_trigger).  The per-trigger arrays share one device buffer and the per-hit and
        per-pulse arrays another (all of 32-bit words), so a chunk comes back in three copies.  The hit arrays hold a hit per
        pulse, which always suffices; the trigger arrays grow to what a call reports, and the call is made again."""
        lib, handle = self.ctx._lib, self.ctx.handle
        n = int(npulses)
        if self._trigger_rows_gpu is None or len(self._trigger_rows_gpu) < nrows + 1:
            self._trigger_rows_gpu = empty(nrows + 1, np.uint32, self.ctx)
        if self._trigger_hits_gpu is None or len(self._trigger_hits_gpu) < 6 * n:
            self._trigger_hits_gpu = empty(6 * n, np.uint32, self.ctx)
        if self._triggers_gpu is None:
            self._triggers_gpu = empty(3 * 1024 + 1, np.uint32, self.ctx)
        per_pulse = [self._trigger_hits_gpu[k * n:(k + 1) * n] for k in range(6)]          # channel, npe, q_int, t_first, flags; pulse_trigger
        trig = trigger.struct()
        ntriggers, nhits = ctypes.c_uint64(0), ctypes.c_uint64(0)
        for attempt in range(2):
            capacity = (len(self._triggers_gpu) - 1) // 3
            per_trigger = [self._triggers_gpu[:capacity], self._triggers_gpu[capacity:2 * capacity], self._triggers_gpu[2 * capacity:3 * capacity + 1]]
            rc = lib.chroma_daq_trigger_pulses(handle, nrows, self.nchannels, ctypes.byref(win), ctypes.byref(trig), d_offsets.ptr,
                                               *([a.ptr for a in arrays] + [n, capacity, self._trigger_rows_gpu.ptr] + [a.ptr for a in per_trigger] +
                                                 [n] + [a.ptr for a in per_pulse] + [ctypes.byref(ntriggers), ctypes.byref(nhits)]))
            if rc == 0 or attempt or ntriggers.value <= capacity:
                break
            grown = int(ntriggers.value) + int(ntriggers.value) // 4
            self._triggers_gpu = empty(3 * grown + 1, np.uint32, self.ctx)
        _lib.check(rc)
        nt, nh = int(ntriggers.value), int(nhits.value)
        self._trigger_device = (self._trigger_rows_gpu, per_trigger[0], per_trigger[2], per_pulse[0], nt, nh)
        t = self._triggers_gpu[:3 * capacity + 1].get()
        h = self._trigger_hits_gpu[:6 * n].get()
        return [self._trigger_rows_gpu[:nrows + 1].get(), t[:nt], t[capacity:capacity + nt], t[2 * capacity:2 * capacity + nt + 1],
                h[:nh].view(np.int32), h[n:n + nh], h[2 * n:2 * n + nh], h[3 * n:3 * n + nh].view(np.float32), h[4 * n:4 * n + nh], h[5 * n:6 * n]]

    def _reduce_slice(self, struct, G, n, d_adc):
        """chroma_daq_reduce_traces on the ``n`` traces a digitise call left in ``d_adc``; the host arrays (found offsets (n + 1,
        uint32), trace base, reduced flags, the arrays of FOUND_COLUMNS).  The pulse arrays grow to what a call reports, and the
        call is made again."""
        lib, handle = self.ctx._lib, self.ctx.handle
        if self._found_rows_gpu is None or len(self._found_rows_gpu) < 3 * n + 1:
            self._found_rows_gpu = empty(3 * n + 1, np.uint32, self.ctx)
        if self._found_gpu is None:
            self._found_gpu = [empty(1024, kind, self.ctx) for _, kind in FOUND_COLUMNS]
        rows = self._found_rows_gpu
        per_trace = [rows[:n + 1], rows[n + 1:2 * n + 1], rows[2 * n + 1:3 * n + 1]]
        nfound = ctypes.c_uint64(0)
        for attempt in range(2):
            capacity = len(self._found_gpu[0])
            rc = lib.chroma_daq_reduce_traces(handle, ctypes.byref(struct), G, n, d_adc.ptr, capacity, *([a.ptr for a in per_trace] +
                                              [a.ptr for a in self._found_gpu] + [ctypes.byref(nfound)]))
            if rc == 0 or attempt or nfound.value <= capacity:
                break
            grown = int(nfound.value) + int(nfound.value) // 4
            self._found_gpu = [empty(grown, kind, self.ctx) for _, kind in FOUND_COLUMNS]
        _lib.check(rc)
        r = rows[:3 * n + 1].get()
        return [r[:n + 1], r[n + 1:2 * n + 1].view(np.int32), r[2 * n + 1:]] + [a[:int(nfound.value)].get() for a in self._found_gpu]

    def _digitize_chunk(self, win, trigger, struct, seed, acquisition, nrows, d_offsets, arrays, npulses, reducer=None, keep_traces=True):
        """chroma_daq_digitize_gates on the pulses, triggers and hits of one chunk where acquire_pulses and _trigger_chunk left
        them, in slices of hits of at most ``max_entries`` samples; the host arrays (adc, trace_flags, found).  With ``reducer`` every
        slice is reduced where it lies, right behind its digitise call (``found``: found offsets (hits + 1, int64), trace base, reduced
        flags and the arrays of FOUND_COLUMNS; None without one); without ``keep_traces`` the samples stay on the device and adc is
        None."""
        lib, handle = self.ctx._lib, self.ctx.handle
        d_trig_offsets, d_trig_bin, d_hit_offsets, d_hit_channel, nt, nh = self._trigger_device
        G = trigger.pre + trigger.post
        per_slice = max(1, self.max_entries // G)
        ntraces = min(nh, per_slice)          # the traces of the largest slice
        if self._adc_gpu is None or len(self._adc_gpu) < ntraces * G:
            self._adc_gpu = empty(ntraces * G, np.uint16, self.ctx)
        if self._trace_flags_gpu is None or len(self._trace_flags_gpu) < ntraces:
            self._trace_flags_gpu = empty(ntraces, np.uint32, self.ctx)
        d_adc, d_flags = self._adc_gpu, self._trace_flags_gpu
        trig = trigger.struct()
        adc, flags = np.zeros((nh, G), dtype=np.uint16) if keep_traces else None, np.zeros(nh, dtype=np.uint32)
        reducer_struct = None if reducer is None else reducer.struct()
        found = [[np.zeros(1, dtype=np.int64)]] + [[] for _ in range(2 + len(FOUND_COLUMNS))]
        nfound = 0
        for first in range(0, nh, per_slice):
            n = min(per_slice, nh - first)
            assert n * G <= len(d_adc) and n <= len(d_flags)          # (the call sees the room for samples only)
            _lib.check(lib.chroma_daq_digitize_gates(handle, nrows, self.nchannels, ctypes.byref(win), ctypes.byref(trig), ctypes.byref(struct), int(seed),
                                                     int(acquisition) & 0xffffffff, d_offsets.ptr, arrays[0].ptr, arrays[1].ptr, arrays[3].ptr, int(npulses),
                                                     d_trig_offsets.ptr, d_trig_bin.ptr, nt, d_hit_offsets.ptr, d_hit_channel.ptr, nh, first, n,
                                                     len(d_adc), d_adc.ptr, d_flags.ptr))
            if keep_traces:
                adc[first:first + n] = d_adc[:n * G].get().reshape(n, G)
            flags[first:first + n] = d_flags[:n].get()
            if reducer is not None:
                got = self._reduce_slice(reducer_struct, G, n, d_adc)
                found[0].append(got[0][1:].astype(np.int64) + nfound)
                for part, a in zip(found[1:], got[1:]):
                    part.append(a)
                nfound += len(got[3])
        if reducer is None:
            return adc, flags, None
        kinds = [np.int64, np.int32, np.uint32] + [kind for _, kind in FOUND_COLUMNS]
        return adc, flags, [np.concatenate(part) if part else np.zeros(0, dtype=kind) for part, kind in zip(found, kinds)]

    def acquire_pulses(self, gpuphotons, rng_states, bounds, window, acquisition=0, weight=1.0, trigger=None, noise=None, digitizer=None,
                       reducer=None, keep_traces=True):
        """The time-binned view of ``acquire`` with the same arguments: the same accepted photons, per (event, channel, bin of
        ``window``: a DaqWindow or (t0, dt, nbins)).  Counts first (chroma_daq_count_pulses), then acquires into buffers grown to
        the largest count seen, ``rows_per_chunk`` events at a time.  Returns an ``EventPulses``.

        ``trigger`` (a DaqTrigger or its tuple): each chunk's pulses are also triggered where they lie on the device, before they
        are read back (chroma_daq_trigger_pulses), and the result carries ``.triggers``, an ``EventTriggers``.  Events are
        independent, so it does not depend on the chunking either; the pulses are what they are without it.

        ``noise`` (a DaqNoise, or a dark rate in Hz, or one per channel): every event's dark-noise photoelectrons are drawn on the
        device and enter the pulses like accepted photons, flagged ``noise.flag`` (chroma_daq_count_pulses_noise /
        chroma_daq_acquire_pulses_noise); the result's ``noise`` counts them per event.  Events without photons get theirs too.
        The draws are counter-based (per event and channel): the chunking does not show.  Noise that is ``off`` is no noise.

        ``digitizer`` (a DaqDigitizer; needs ``trigger``): each chunk's gated hits are also digitised where they lie on the device,
        after its trigger call (chroma_daq_digitize_gates, in slices of hits of at most ``max_entries`` samples), and ``.triggers``
        carries ``adc`` and ``trace_flags``.  The electronics noise is counter-based too (per event, channel and bin).

        ``reducer`` (a DaqReducer or its tuple; needs ``digitizer``): every digitised slice is also reduced where it lies, right behind
        its digitise call (chroma_daq_reduce_traces), and ``.triggers`` carries the found pulses (``found_offsets``, ``found_*``,
        ``trace_base``, ``reduced_flags``, ``reducer``).  With ``keep_traces=False`` the samples are not copied to the host:
        ``triggers.adc`` is None, ``trace_flags`` still comes back."""
        window = DaqWindow.of(window)
        if reducer is not None:
            if digitizer is None:
                raise ValueError('a reducer reads the traces of a digitiser: reducer needs digitizer')
            reducer = DaqReducer.of(reducer)
        if digitizer is not None:
            if trigger is None:
                raise ValueError('a digitiser reads the gates of a trigger: digitizer needs trigger')
            digitizer = DaqDigitizer.of(digitizer)
        if noise is not None:
            noise = DaqNoise.of(noise)
            noise = None if noise.off else noise
        if trigger is not None:
            trigger = DaqTrigger.of(trigger).check(window)
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
        if digitizer is not None:
            digitizer.check(trigger)
            if reducer is not None:
                reducer.check(trigger.pre + trigger.post)
            digitizer_struct, digitizer_arrays = digitizer.struct(self.charge_unit)
            # the electronics noise draws from the pseudo-photons 0xffffffff00000000 | channel, as the dark noise does
            n_ids, base = len(gpuphotons.pos), int(rng.photon_id_base)
            if digitizer.noise_sigma > 0.0 and n_ids and ((base >> 32) == 0xffffffff or ((base + n_ids - 1) >> 32) >= 0xffffffff):
                raise ValueError('the photon ids reach the high word 0xffffffff of the noise\'s pseudo-photons')
            traces = [[], []]
            found = [[np.zeros(1, dtype=np.int64)]] + [[] for _ in range(2 + len(FOUND_COLUMNS))]
            nfound = 0
        noise_arg = () if noise is None else (ctypes.byref(self._noise_struct(noise, window)),)
        suffix = '' if noise is None else '_noise'
        offsets, outside, row_noise = [np.zeros(1, dtype=np.int64)], [], []
        parts = [[] for _ in range(6)]
        total = 0
        triggered = [[np.zeros(1, dtype=np.int64)] if k in (0, 3) else [] for k in range(10)]
        ntriggers = nhits = 0
        for first in range(0, nevents, self.rows_per_chunk):
            nrows = min(self.rows_per_chunk, nevents - first)
            b = bounds[first:first + nrows + 1]
            args = (handle, self.gpu_detector.handle, ctypes.byref(self.tables), nrows, _lib.ptr(b), event.SURFACE_DETECT, ctypes.byref(s),
                    len(gpuphotons.pos), rng, (int(acquisition) + first) & 0xffffffff, float(weight), ctypes.byref(win)) + noise_arg
            naccepted = ctypes.c_uint64(0)
            _lib.check(getattr(lib, 'chroma_daq_count_pulses' + suffix)(*(args + (ctypes.byref(naccepted),))))
            capacity = int(naccepted.value)
            (d_offsets, d_outside, d_row_noise), arrays = self._pulse_buffers(nrows, capacity)
            npulses = ctypes.c_uint64(0)
            _lib.check(getattr(lib, 'chroma_daq_acquire_pulses' + suffix)(*(args + (capacity, d_offsets.ptr) + tuple(a.ptr for a in arrays) +
                                                                             (d_outside.ptr,) + (() if noise is None else (d_row_noise.ptr,)) +
                                                                             (ctypes.byref(npulses),))))
            if noise is not None:
                row_noise.append(d_row_noise[:nrows].get())
            offsets.append(d_offsets[:nrows + 1].get()[1:].astype(np.int64) + total)
            outside.append(d_outside[:2 * nrows].get().reshape(nrows, 2))
            for part, a in zip(parts, arrays):
                part.append(a[:npulses.value].get())
            if trigger is not None:
                got = self._trigger_chunk(win, trigger, nrows, d_offsets, arrays, int(npulses.value))
                triggered[0].append(got[0][1:].astype(np.int64) + ntriggers)
                triggered[3].append(got[3][1:].astype(np.int64) + nhits)
                triggered[9].append(np.where(got[9] == NO_TRIGGER, got[9], got[9] + np.uint32(ntriggers & 0xffffffff)).astype(np.uint32))
                for k in (1, 2, 4, 5, 6, 7, 8):
                    triggered[k].append(got[k])
                ntriggers += len(got[1])
                nhits += len(got[4])
                if digitizer is not None:
                    adc, flags, got = self._digitize_chunk(win, trigger, digitizer_struct, rng.seed, int(acquisition) + first, nrows, d_offsets,
                                                           arrays, int(npulses.value), reducer=reducer, keep_traces=keep_traces)
                    traces[0].append(adc)
                    traces[1].append(flags)
                    if got is not None:
                        found[0].append(got[0][1:] + nfound)
                        for part, a in zip(found[1:], got[1:]):
                            part.append(a)
                        nfound += len(got[3])
            total += int(npulses.value)
        dtypes = (np.int32, np.uint32, np.uint32, np.uint32, np.float32, np.uint32)
        columns = [np.concatenate(part) if part else np.zeros(0, dtype=dtype) for part, dtype in zip(parts, dtypes)]
        outside = np.concatenate(outside) if outside else np.zeros((0, 2), dtype=np.uint32)
        pulses = EventPulses(window, self.nchannels, self.charge_unit, np.concatenate(offsets), *columns, outside=outside,
                             noise=np.concatenate(row_noise) if row_noise else None)
        if trigger is not None:
            kinds = (np.int64, np.uint32, np.uint32, np.int64, np.int32, np.uint32, np.uint32, np.float32, np.uint32, np.uint32)
            pulses.triggers = EventTriggers(window, trigger, self.nchannels, self.charge_unit, pulses.offsets,
                                            *[np.concatenate(part) if part else np.zeros(0, dtype=dtype) for part, dtype in zip(triggered, kinds)],
                                            pulses=(pulses.channel, pulses.bin, pulses.q_int))
            if digitizer is not None:
                G = trigger.pre + trigger.post
                if keep_traces:
                    pulses.triggers.adc = np.concatenate(traces[0]) if traces[0] else np.zeros((0, G), dtype=np.uint16)
                pulses.triggers.trace_flags = np.concatenate(traces[1]) if traces[1] else np.zeros(0, dtype=np.uint32)
                pulses.triggers.digitizer = digitizer
                if reducer is not None:
                    kinds = [np.int64, np.int32, np.uint32] + [kind for _, kind in FOUND_COLUMNS]
                    got = [np.concatenate(part) if part else np.zeros(0, dtype=kind) for part, kind in zip(found, kinds)]
                    _set_found(pulses.triggers, (reducer, got[0], got[1], got[2], got[3:]))
        return pulses
