"""The result containers of the DAQ -- ``EventChannels``; ``EventPulses`` and per event ``Pulses``; ``EventTriggers`` and per event
``Triggers``, with ``FoundPulses`` -- and the host twins that build them without a GPU: ``trigger_pulses_host`` (NumPy),
``EventTriggers.digitize`` (chroma_daq_digitize_host) and ``reduce_traces_host`` (chroma_daq_reduce_host)."""
import ctypes

import numpy as np

from chroma_amd import _lib, event
from chroma_amd.gpu.daq.records import (FIRING_COLUMNS, HIT_COLUMNS, FOUND_COLUMNS, REDUCED_COLUMNS, NO_TRIGGER, names, named, zeros_of,
                                        rebase_triggers, count_then_fill, index_of)
from chroma_amd.gpu.daq.settings import DaqTrigger, DaqDigitizer, DaqReducer


def dense_channels(nchannels, channel, t, q, flags):
    """The dense ``event.Channels`` of ``nchannels`` channels from the sparse columns of those that hold something: t = 1e9, no
    charge and no flags elsewhere; as in the reference, a channel whose time is still the reset value (1e9) was not hit."""
    dense_t = np.full(nchannels, 1e9, dtype=np.float32)
    dense_q = np.zeros(nchannels, dtype=np.float32)
    dense_flags = np.zeros(nchannels, dtype=np.uint32)
    dense_t[channel] = t
    dense_q[channel] = q
    dense_flags[channel] = flags
    return event.Channels(dense_t < 1e8, dense_t, dense_q, dense_flags)


def _channel_of(channel, nchannels):
    channel = int(channel)
    if not 0 <= channel < nchannels:
        raise IndexError('channel %d of %d' % (channel, nchannels))
    return channel


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
        i = index_of(i, self.nevents, 'event')
        offsets, channel, t, q, flags = self._chunks[i // self.rows_per_chunk]
        row = i % self.rows_per_chunk
        w = slice(int(offsets[row]), int(offsets[row + 1]))
        return channel[w], t[w], q[w], flags[w]

    def __getitem__(self, i):
        """The dense ``event.Channels`` of event ``i``, bit for bit what ``GPUDaq.end_acquire().get()`` gives for it."""
        return dense_channels(self.nchannels, *self.sparse(i))


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
        channel = _channel_of(channel, self.nchannels)
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

    def _slice(self, i):
        i = index_of(i, self.nevents, 'event')
        return slice(int(self.offsets[i]), int(self.offsets[i + 1]))

    def sparse(self, i):
        """(channel, bin, npe, q, t_first, flags) of event ``i``, as slices (no copy); q = float32(q_int) * charge_unit."""
        w = self._slice(i)
        return self.channel[w], self.bin[w], self.npe[w], self.q[w], self.t_first[w], self.flags[w]

    def outside(self, i):
        """(early, late): the accepted photons of event ``i`` before t0 and behind the last bin."""
        early, late = self._outside[index_of(i, self.nevents, 'event')]
        return int(early), int(late)

    def event(self, i):
        """The ``Pulses`` of event ``i``: views of this object's arrays."""
        w = self._slice(i)
        early, late = self.outside(i)
        return Pulses(self.window, self.nchannels, self.channel[w], self.bin[w], self.npe[w], self.q[w], self.q_int[w], self.t_first[w],
                      self.flags[w], early, late, int(self.noise[index_of(i, self.nevents, 'event')]))

    def waveform(self, i, channel):
        """(npe[nbins] uint32, q[nbins] float32) of one channel of event ``i``, dense."""
        return self.event(i).waveform(channel)

    def trigger(self, trigger):
        """The ``EventTriggers`` of these pulses under ``trigger`` (a DaqTrigger or its tuple), computed in NumPy on the host
        arrays -- no GPU, no library: what ``GPUEventDaq.acquire_pulses(trigger=...)`` computes on the device, bit for bit."""
        return trigger_pulses_host(self.window, trigger, self.nchannels, self.charge_unit, self.offsets, self.channel, self.bin, self.npe,
                                   self.q_int, self.t_first, self.flags)


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
    offsets = np.zeros(ntraces + 1, dtype=np.uint32)
    per_trace = zeros_of(REDUCED_COLUMNS, ntraces)
    nfound = ctypes.c_uint64(0)
    columns = []

    def call(capacity):
        columns[:] = zeros_of(FOUND_COLUMNS, capacity)
        rc = lib.chroma_daq_reduce_host(ctypes.byref(struct), G, ntraces, _lib.ptr(adc), capacity, _lib.ptr(offsets),
                                        *([_lib.ptr(a) for a in per_trace] + [_lib.ptr(a) if capacity else None for a in columns] + [ctypes.byref(nfound)]))
        return rc, nfound.value
    count_then_fill(call, 0)
    return [offsets.astype(np.int64)] + per_trace + [a[:int(nfound.value)] for a in columns]


# what a trace reduction adds to a ``Triggers`` or an ``EventTriggers``; their ``found`` is {name: value} of these, or None
FOUND_FIELDS = ('reducer', 'found_offsets') + names(REDUCED_COLUMNS) + names(FOUND_COLUMNS)


def _set_found(self, found):
    for name in FOUND_FIELDS:
        setattr(self, name, None if found is None else found[name])


def _found(self, h=None):
    """The ``found`` of ``self``; with ``h`` (a slice of hits) that of those hits, the offsets rebased to 0."""
    if self.reducer is None:
        return None
    found = {name: getattr(self, name) for name in FOUND_FIELDS}
    if h is not None:
        f = slice(int(self.found_offsets[h.start]), int(self.found_offsets[h.stop]))
        found.update({name: found[name][h] for name in names(REDUCED_COLUMNS)}, **{name: found[name][f] for name in names(FOUND_COLUMNS)})
        found['found_offsets'] = self.found_offsets[h.start:h.stop + 1] - self.found_offsets[h.start]
    return found


class FoundPulses(object):
    """The pulses found in ONE trace (``Triggers.found``): the arrays of ``FOUND_COLUMNS`` without their prefix (``start``,
    ``width``, ``peak``, ``peak_sample``, ``integral``, ``time``, ``flags``), ``t`` (ns, float64) and ``q`` (float64: the detector's
    charge units where the reducer knows a gain, else ADC counts x samples)."""

    def __init__(self, columns, t, q):
        for name, a in zip(names(FOUND_COLUMNS), columns):
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
        self.vertices = None          # (Simulation(daq_seeder=...): the ``chroma_amd.seed.SeedFits`` of the firings)
        self.directions = None        # (Simulation(daq_direction=...): the ``chroma_amd.seed.DirFits`` of the firings)

    def __len__(self):
        return len(self.bin)

    def seed_rows(self, k, source='reco'):
        """(channel, t, weight) of firing ``k`` as a vertex seed takes them: 'reco' -- ``reco(k)``'s channels, times and charges
        (raises as ``reco`` does without a reducer); 'gate' -- the gate's channels, earliest times and photoelectrons."""
        if source == 'reco':
            return self.reco(k)[:3]
        if source == 'gate':
            channel, npe, _, t, _ = self.sparse(k)
            return channel, t, npe
        raise ValueError("source: 'reco' or 'gate'")

    def seed(self, k, seeder, source='reco'):
        """The ``SeedFits`` (one fit) of firing ``k`` under the ``chroma_amd.seed.VertexSeeder`` ``seeder``, on the host."""
        return seeder.fit(*self.seed_rows(k, source))

    def direction(self, k, seeder, vertex, source='reco'):
        """The ``DirFits`` (one fit) of firing ``k`` under the ``chroma_amd.seed.DirectionSeeder`` ``seeder`` about ``vertex`` (the
        firing's ``SeedFits``: ``seed(k, ...)``, or ``vertices[k:k + 1]``), on the host."""
        return seeder.fit(vertex, *self.seed_rows(k, source))

    def adc(self, k):
        """(channel, traces) of firing ``k``: the channels read out, ascending, and their traces (len(channel) x (pre + post),
        uint16), as slices (no copy)."""
        if self.traces is None:
            raise ValueError('these triggers were not digitised (daq_digitizer / digitizer=...)')
        w = self._slice(k)
        return self.hit_channel[w], self.traces[w]

    def _hit_of(self, k, channel):
        """the hit of ``channel`` in firing ``k``; KeyError for a channel without a pulse in the gate"""
        w = self._slice(k)
        channel = _channel_of(channel, self.nchannels)
        at = w.start + int(np.searchsorted(self.hit_channel[w], channel))
        if at == w.stop or self.hit_channel[at] != channel:
            raise KeyError('channel %d has no pulse in the gate of firing %d' % (channel, k))
        return at

    def trace(self, k, channel):
        """The trace of ``channel`` in firing ``k``; KeyError for a channel without a pulse in the gate: it was not read out."""
        self.adc(k)
        return self.traces[self._hit_of(k, channel)]

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
        at = self._hit_of(k, channel)
        f = self._found_of(slice(at, at + 1))
        columns = [getattr(self, name)[f] for name in names(FOUND_COLUMNS)]
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
        channel, t, q, _, flags = self.reco(k)
        return dense_channels(self.nchannels, channel, t, q, flags)

    @property
    def time(self):
        """The nominal lower edge t0 + bin dt of every firing's bin (float64)."""
        return self.window.t0 + self.window.dt * self.bin.astype(np.float64)

    def _slice(self, k):
        k = index_of(k, len(self), 'trigger')
        return slice(int(self.hit_offsets[k]), int(self.hit_offsets[k + 1]))

    def sparse(self, k):
        """(channel, npe, q, t_first, flags) of the gate of firing ``k``, in channel order, as slices (no copy)."""
        w = self._slice(k)
        return self.hit_channel[w], self.hit_npe[w], self.hit_q[w], self.hit_t_first[w], self.hit_flags[w]

    def channels(self, k):
        """The dense ``event.Channels`` of the gate of firing ``k``: a channel's earliest time and charge in the gate, built as
        ``EventChannels.__getitem__`` builds an event's (t = 1e9 and not hit where the gate holds nothing of the channel)."""
        channel, npe, q, t, flags = self.sparse(k)
        return dense_channels(self.nchannels, channel, t, q, flags)


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

    FIELDS = (('window', 'trigger', 'nchannels', 'charge_unit', 'pulse_offsets', 'offsets') + names(FIRING_COLUMNS) + ('hit_offsets',) +
              names(HIT_COLUMNS) + ('pulse_trigger', 'adc', 'trace_flags', 'digitizer', 'pulses'))

    def replace(self, **fields):
        """A new ``EventTriggers`` over the same arrays, with ``fields`` (arguments of the constructor, by name) in place of this one's."""
        kw = dict({name: getattr(self, name) for name in self.FIELDS}, found=_found(self))
        kw.update(fields)
        return EventTriggers(**kw)

    def digitize(self, digitizer, seed=0, acquisition=0):
        """These triggers with the traces of their gated hits under ``digitizer``, computed on the HOST (chroma_daq_digitize_host: no
        GPU) from the pulses and triggers held here -- bit for bit what ``GPUEventDaq.acquire_pulses(trigger=..., digitizer=digitizer,
        acquisition=acquisition)`` reads back on a context seeded with ``seed``.  Event i is acquisition ``acquisition + i``.  Returns
        a new ``EventTriggers`` over the same arrays, not reduced."""
        digitizer = DaqDigitizer.of(digitizer).check(self.trigger)
        if self.pulses is None:
            raise ValueError('these triggers do not hold their pulses')
        lib = _lib.load()
        struct, keep = digitizer.struct(self.charge_unit)
        win = self.window.struct()
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
        return self.replace(adc=adc, trace_flags=trace_flags, digitizer=digitizer, found=None)

    def reduce(self, reducer):
        """These triggers with the pulses found in their traces under ``reducer``, computed on the HOST (chroma_daq_reduce_host: no
        GPU) from the ``adc`` held here -- bit for bit what ``GPUEventDaq.acquire_pulses(..., reducer=reducer)`` reads back.  Returns
        a new ``EventTriggers`` over the same arrays."""
        if self.adc is None:
            raise ValueError('these triggers hold no traces (daq_digitizer / digitizer=... with keep_traces, or digitize)')
        reducer = DaqReducer.of(reducer)
        return self.replace(found=dict(zip(FOUND_FIELDS, [reducer] + reduce_traces_host(self.adc, reducer))))

    def seed(self, seeder, source='reco', gpu=None):
        """The ``chroma_amd.seed.SeedFits`` of EVERY firing of the batch, in firing order, under the ``VertexSeeder`` ``seeder``, in ONE
        call: on the host (``gpu`` None: chroma_vertex_seed_host) or on the device (``gpu``: a ``chroma_amd.gpu.seed.GPUVertexSeeder``
        or a context) -- the same bits.  ``source`` as ``Triggers.seed_rows``.  The fits of event i are [offsets[i], offsets[i + 1])."""
        return seeder.fit_many(*self.seed_rows(source), gpu=gpu)

    def seed_rows(self, source='reco'):
        """(offsets, channel, t, weight) of EVERY firing of the batch, in firing order, as ``fit_many`` takes them."""
        if source == 'reco' and self.reducer is None:
            raise ValueError('these triggers were not reduced (daq_reducer / reducer=... / reduce)')
        rows = []
        for i in range(self.nevents):
            triggers = self.event(i)
            rows.extend(triggers.seed_rows(k, source) for k in range(len(triggers)))
        offsets = np.concatenate([[0], np.cumsum([len(r[0]) for r in rows], dtype=np.int64)]).astype(np.int64)
        column = lambda j, kind: np.concatenate([np.asarray(r[j], dtype=kind) for r in rows]) if rows else np.zeros(0, dtype=kind)
        return offsets, column(0, np.int32), column(1, np.float64), column(2, np.float64)

    def direction(self, seeder, vertices, source='reco', gpu=None):
        """The ``chroma_amd.seed.DirFits`` of EVERY firing of the batch, in firing order, under the ``DirectionSeeder`` ``seeder`` about
        ``vertices`` (the ``SeedFits`` of ``seed(...)`` with the same source), in ONE call: on the host (``gpu`` None:
        chroma_direction_seed_host) or on the device (a ``chroma_amd.gpu.seed.GPUDirectionSeeder`` or a context) -- the same bits."""
        return seeder.fit_many(vertices, *self.seed_rows(source), gpu=gpu)

    def __len__(self):
        return self.nevents

    def event(self, i):
        """The ``Triggers`` of event ``i``."""
        i = index_of(i, self.nevents, 'event')
        a, b = int(self.offsets[i]), int(self.offsets[i + 1])
        h = slice(int(self.hit_offsets[a]), int(self.hit_offsets[b]))
        columns = {name: getattr(self, name)[a:b] for name in names(FIRING_COLUMNS)}
        columns.update({name: getattr(self, name)[h] for name in names(HIT_COLUMNS)})
        return Triggers(self.window, self.trigger, self.nchannels, self.charge_unit, hit_offsets=self.hit_offsets[a:b + 1] - self.hit_offsets[a],
                        pulse_trigger=rebase_triggers(self.pulse_trigger[int(self.pulse_offsets[i]):int(self.pulse_offsets[i + 1])], -a),
                        adc=None if self.adc is None else self.adc[h], trace_flags=None if self.trace_flags is None else self.trace_flags[h],
                        digitizer=self.digitizer, found=_found(self, h), **columns)


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
    hits = named(HIT_COLUMNS, [(hit_key % nch).astype(np.int32), hit_npe.astype(np.uint32), hit_q.astype(np.uint32), hit_t.view(np.float32),
                               hit_flags.astype(np.uint32)])
    return EventTriggers(window, trigger, nch, charge_unit, offsets, trig_offsets.astype(np.int64), t_bin.astype(np.uint32),
                         t_sum.astype(np.uint32), hit_offsets.astype(np.int64), pulse_trigger=pulse_trigger, pulses=(channel, bin, q_int), **hits)
