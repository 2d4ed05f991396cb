"""The device drivers of the DAQ: ``GPUDaq`` / ``GPUChannels`` (one acquisition, or ``ndaq`` side by side) and ``GPUEventDaq`` (the
acquisitions, pulses, triggers, traces and found pulses of a whole batch, a chunk of events at a time)."""
import collections
import ctypes

import numpy as np

from chroma_amd import _lib, event
from chroma_amd.gpu.tools import empty, zeros, to_gpu
from chroma_amd.gpu.photon import _structure
from chroma_amd.gpu.daq.records import (PULSE_COLUMNS, FIRING_COLUMNS, HIT_COLUMNS, FOUND_COLUMNS, REDUCED_COLUMNS, names, kinds, named,
                                        columns_of, Columns, Ragged, rebase_triggers, count_then_fill)
from chroma_amd.gpu.daq.settings import DaqWindow, DaqChain, daq_needs, _padded_cdf
from chroma_amd.gpu.daq.results import EventChannels, EventPulses, EventTriggers


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
        lib = self.ctx._lib
        call, copies = (lib.chroma_daq_acquire, ()) if self.ndaq == 1 else (lib.chroma_daq_acquire_many, (int(self.ndaq), int(self.stride)))
        _lib.check(call(self.ctx.handle, self.gpu_detector.handle, ctypes.byref(self.tables), int(start_photon), int(nphotons), event.SURFACE_DETECT,
                        ctypes.byref(s), rng, self.acquisition, float(weight), *(copies + (self.earliest_time_int_gpu.ptr, self.channel_q_int_gpu.ptr,
                                                                                           self.channel_history_gpu.ptr))))
        self.acquisition += 1
        self.ctx.synchronize()

    def end_acquire(self, nthreads_per_block=64):
        _lib.check(self.ctx._lib.chroma_daq_convert(self.ctx.handle, len(self.earliest_time_int_gpu), self.charge_unit,
                                                    self.earliest_time_int_gpu.ptr, self.channel_q_int_gpu.ptr,
                                                    self.earliest_time_gpu.ptr, self.channel_q_gpu.ptr))
        self.ctx.synchronize()
        return GPUChannels(self.earliest_time_gpu, self.channel_q_gpu, self.channel_history_gpu, self.ndaq, self.stride)


def _photon_bounds(bounds):
    """``bounds`` as the contiguous uint32 array the library reads, or ValueError."""
    bounds = np.asarray(bounds)
    if bounds.ndim != 1 or len(bounds) < 1 or not np.issubdtype(bounds.dtype, np.integer):
        raise ValueError('bounds: a 1-D array of at least one photon index')
    if len(bounds) and (bounds.min() < 0 or bounds.max() > 0xffffffff):
        raise ValueError('bounds: photon indices of 32 bits')
    return np.ascontiguousarray(bounds, dtype=np.uint32)


# what a trigger call leaves on the device for the digitiser: the firings' offsets per row and their bins, the hits' offsets per
# firing and their channels, and the numbers of firings and hits
Fired = collections.namedtuple('Fired', 'offsets bin hit_offsets hit_channel nt nh')

# what acquire_pulses says in front of a stage that is given without the one it needs
_WHY = {'reducer': 'a reducer reads the traces of a digitiser: ', 'digitizer': 'a digitiser reads the gates of a trigger: '}


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
        self._noise_tables = None            # acquire_pulses(noise=...): ((noise, window), the chroma_daq_noise, its arrays), the last one
        # the outputs on the device, each made on first use and grown to the largest request seen (_room):
        self._offsets_gpu = self._sparse_gpu = None                                        # the compaction's: per row; per touched word
        self._pulse_offsets_gpu = self._pulse_outside_gpu = self._pulse_noise_gpu = None   # acquire_pulses': per row ...
        self._pulses_gpu = None                                                            # ... and per pulse the PULSE_COLUMNS
        self._trigger_rows_gpu = None        # trigger=...: per row the offsets; per firing (bin, sum, hit offsets) in one buffer;
        self._triggers_gpu = None            # per hit the HIT_COLUMNS and per pulse its trigger in another (all 32-bit words)
        self._trigger_hits_gpu = None
        self._adc_gpu = None                 # digitizer=...: the samples of one slice of hits ...
        self._trace_flags_gpu = None         # ... and its flag words, each grown on its own (a shorter gate: fewer samples, more traces)
        self._found_rows_gpu = None          # reducer=...: per trace of a slice (offsets + 1, base, flags) in one buffer ...
        self._found_gpu = None               # ... and per found pulse the FOUND_COLUMNS, grown to what a call reports

    def _room(self, name, n, kind=np.uint32):
        """The device buffer ``self.<name>`` with room for ``n`` entries of ``kind`` -- or, for a list of kinds, the list of one
        buffer each: made anew with ``n`` entries (not copied) when there is none yet or a shorter one."""
        held = getattr(self, name)
        many = isinstance(kind, list)
        if held is None or len(held[0] if many else held) < n:
            held = [empty(n, k, self.ctx) for k in kind] if many else empty(n, kind, self.ctx)
            setattr(self, name, held)
        return held

    def acquire(self, gpuphotons, rng_states, bounds, acquisition=0, weight=1.0):
        """One acquisition per event of ``bounds`` (len(events) + 1 ascending photon indices into ``gpuphotons``; event r is
        the photons [bounds[r], bounds[r + 1]), empty events allowed), event r as acquisition ``acquisition + r``.  Returns
        an ``EventChannels``."""
        bounds = _photon_bounds(bounds)
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
            offsets = self._room('_offsets_gpu', nrows + 1)
            sparse = self._room('_sparse_gpu', capacity, [np.int32, np.float32, np.float32, np.uint32])
            ntouched = ctypes.c_uint64(0)
            _lib.check(lib.chroma_daq_compact_events(handle, nrows, nch, nch, self.charge_unit, *accumulators, capacity,
                                                     offsets.ptr, *[a.ptr for a in sparse], ctypes.byref(ntouched)))
            chunks.append(tuple([offsets[:nrows + 1].get()] + [a[:ntouched.value].get() for a in sparse]))
        return EventChannels(nch, nevents, self.rows_per_chunk, chunks)

    def _noise_struct(self, noise, window):
        """The chroma_daq_noise of ``noise`` under ``window`` on this context: built and uploaded once per (noise, window)."""
        key = (noise, window)
        if self._noise_tables is None or self._noise_tables[0] != key:
            count_cdf, accept = noise.tables(window, self.nchannels)
            d_accept = to_gpu(accept, ctx=self.ctx)
            self._noise_tables = (key, _lib.DaqNoise(_lib.ptr(count_cdf), len(count_cdf), d_accept.ptr, noise.flag), (count_cdf, d_accept))
        return self._noise_tables[1]

    def _trigger_chunk(self, win, trigger, nrows, d_offsets, arrays, n):
        """chroma_daq_trigger_pulses on the ``n`` pulses of one chunk where acquire_pulses left them.  Returns the host arrays by
        name -- the firings' ``offsets`` and FIRING_COLUMNS, the hits' ``hit_offsets`` and HIT_COLUMNS, ``pulse_trigger`` -- and the
        ``Fired`` left on the device.  The per-firing arrays share one device buffer and the per-hit and per-pulse arrays
        another (all of 32-bit words), so a chunk comes back in three copies.  The hit arrays hold a hit per pulse, which always
        suffices; the firing arrays grow to what a call reports, and the call is made again."""
        lib, handle = self.ctx._lib, self.ctx.handle
        d_rows = self._room('_trigger_rows_gpu', nrows + 1)
        d_hits = self._room('_trigger_hits_gpu', 6 * n)
        per_pulse = [d_hits[k * n:(k + 1) * n] for k in range(6)]          # the HIT_COLUMNS, then pulse_trigger
        trig = trigger.struct()
        ntriggers, nhits = ctypes.c_uint64(0), ctypes.c_uint64(0)
        per_firing = []

        def call(capacity):
            d = self._room('_triggers_gpu', 3 * capacity + 1)
            per_firing[:] = [d[:capacity], d[capacity:2 * capacity], d[2 * capacity:3 * capacity + 1]]          # bin, sum; hit offsets
            rc = lib.chroma_daq_trigger_pulses(handle, nrows, self.nchannels, ctypes.byref(win), ctypes.byref(trig), d_offsets.ptr,
                                               *([a.ptr for a in arrays] + [n, capacity, d_rows.ptr] + [a.ptr for a in per_firing] +
                                                 [n] + [a.ptr for a in per_pulse] + [ctypes.byref(ntriggers), ctypes.byref(nhits)]))
            return rc, ntriggers.value
        held = 1024 if self._triggers_gpu is None else (len(self._triggers_gpu) - 1) // 3
        nt, capacity = count_then_fill(call, held, spare=True)
        nh = int(nhits.value)
        t = self._triggers_gpu[:3 * capacity + 1].get()
        h = d_hits[:6 * n].get()
        got = dict(offsets=d_rows[:nrows + 1].get(), hit_offsets=t[2 * capacity:2 * capacity + nt + 1], pulse_trigger=h[5 * n:6 * n])
        got.update(named(FIRING_COLUMNS + HIT_COLUMNS, [t[:nt], t[capacity:capacity + nt]] +
                         [h[k * n:k * n + nh].view(kind) for k, kind in enumerate(kinds(HIT_COLUMNS))]))
        return got, Fired(d_rows, per_firing[0], per_firing[2], per_pulse[0], nt, nh)

    def _reduce_slice(self, struct, G, n, d_adc):
        """chroma_daq_reduce_traces on the ``n`` traces a digitise call left in ``d_adc``; the host arrays by name: ``found_offsets``
        (n + 1, uint32), the REDUCED_COLUMNS and the FOUND_COLUMNS.  The pulse arrays grow to what a call reports, and the call is
        made again."""
        lib, handle = self.ctx._lib, self.ctx.handle
        rows = self._room('_found_rows_gpu', 3 * n + 1)
        per_trace = [rows[:n + 1], rows[n + 1:2 * n + 1], rows[2 * n + 1:3 * n + 1]]
        nfound = ctypes.c_uint64(0)

        def call(capacity):
            d_found = self._room('_found_gpu', capacity, kinds(FOUND_COLUMNS))
            rc = lib.chroma_daq_reduce_traces(handle, ctypes.byref(struct), G, n, d_adc.ptr, capacity, *([a.ptr for a in per_trace] +
                                              [a.ptr for a in d_found] + [ctypes.byref(nfound)]))
            return rc, nfound.value
        count, _ = count_then_fill(call, 1024 if self._found_gpu is None else len(self._found_gpu[0]), spare=True)
        r = rows[:3 * n + 1].get()
        got = dict(named(REDUCED_COLUMNS, [r[n + 1:2 * n + 1].view(np.int32), r[2 * n + 1:]]), found_offsets=r[:n + 1])
        got.update(named(FOUND_COLUMNS, [a[:count].get() for a in self._found_gpu]))
        return got

    def _digitize_chunk(self, win, trigger, struct, seed, acquisition, nrows, d_offsets, arrays, npulses, fired, per_hit, found, reducer, keep_traces):
        """chroma_daq_digitize_gates on the pulses of one chunk where acquire_pulses left them and on what its trigger call left
        (``fired``), in slices of hits of at most ``max_entries`` samples.  Every slice is appended to ``per_hit``: its ``adc`` (only
        with ``keep_traces``: else the samples stay on the device) and ``trace_flags``.  With ``reducer`` every slice is reduced where it
        lies, right behind its digitise call: its REDUCED_COLUMNS go to ``per_hit`` too and its found pulses to ``found``."""
        lib, handle = self.ctx._lib, self.ctx.handle
        G = trigger.pre + trigger.post
        per_slice = max(1, self.max_entries // G)
        ntraces = min(fired.nh, per_slice)          # the traces of the largest slice
        d_adc = self._room('_adc_gpu', ntraces * G, np.uint16)
        d_flags = self._room('_trace_flags_gpu', ntraces)
        trig = trigger.struct()
        reducer_struct = None if reducer is None else reducer.struct()
        for first in range(0, fired.nh, per_slice):
            n = min(per_slice, fired.nh - first)
            assert n * G <= len(d_adc) and n <= len(d_flags)          # (the call sees the room for samples only)
            _lib.check(lib.chroma_daq_digitize_gates(handle, nrows, self.nchannels, ctypes.byref(win), ctypes.byref(trig), ctypes.byref(struct), int(seed),
                                                     int(acquisition) & 0xffffffff, d_offsets.ptr, arrays[0].ptr, arrays[1].ptr, arrays[3].ptr, int(npulses),
                                                     fired.offsets.ptr, fired.bin.ptr, fired.nt, fired.hit_offsets.ptr, fired.hit_channel.ptr, fired.nh,
                                                     first, n, len(d_adc), d_adc.ptr, d_flags.ptr))
            columns = [d_adc[:n * G].get().reshape(n, G)] if keep_traces else []
            columns.append(d_flags[:n].get())
            if reducer is not None:
                got = self._reduce_slice(reducer_struct, G, n, d_adc)
                columns += columns_of(REDUCED_COLUMNS, got)
                found.append(got['found_offsets'], columns_of(FOUND_COLUMNS, got))
            per_hit.append(columns)

    def acquire_pulses(self, gpuphotons, rng_states, bounds, window, acquisition=0, weight=1.0, trigger=None, noise=None, digitizer=None,
                       reducer=None, keep_traces=True, chain=None):
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
        ``triggers.adc`` is None, ``trace_flags`` still comes back.

        ``chain`` (a DaqChain): the readout, resolved by the caller; ``window`` and the five keywords above are then not looked at,
        and nothing is converted or checked again."""
        if chain is None:
            window = DaqWindow.of(window)
            daq_needs(dict(window=window, trigger=trigger, digitizer=digitizer, reducer=reducer), stages=('reducer', 'digitizer'), reasons=_WHY)
            chain = DaqChain(window, trigger, noise, digitizer, reducer, keep_traces)
        window, trigger, noise, digitizer, reducer, keep_traces = (chain.window, chain.trigger, chain.noise, chain.digitizer, chain.reducer,
                                                                   chain.keep_traces)
        bounds = _photon_bounds(bounds)
        nevents = len(bounds) - 1
        rng = gpuphotons._rng(rng_states)
        s = _structure(gpuphotons)
        lib, handle = self.ctx._lib, self.ctx.handle
        win = window.struct()
        if digitizer is not None:
            G = trigger.pre + trigger.post
            digitizer_struct, digitizer_arrays = digitizer.struct(self.charge_unit)
            # the electronics noise draws from the pseudo-photons 0xffffffff00000000 | channel, as the dark noise does
            n_ids, base = len(gpuphotons.pos), int(rng.photon_id_base)
            if digitizer.noise_sigma > 0.0 and n_ids and ((base >> 32) == 0xffffffff or ((base + n_ids - 1) >> 32) >= 0xffffffff):
                raise ValueError('the photon ids reach the high word 0xffffffff of the noise\'s pseudo-photons')
            per_hit = Columns(((('adc', (np.uint16, (G,))),) if keep_traces else ()) + (('trace_flags', np.uint32),) +
                              (REDUCED_COLUMNS if reducer is not None else ()))
            found = Ragged(FOUND_COLUMNS)          # (rows: the traces)
        noise_arg = () if noise is None else (ctypes.byref(self._noise_struct(noise, window)),)
        suffix = '' if noise is None else '_noise'
        per_row = Columns((('outside', (np.uint32, (2,))),) + (() if noise is None else (('noise', np.uint32),)))
        pulses, firings, hits = Ragged(PULSE_COLUMNS), Ragged(FIRING_COLUMNS), Ragged(HIT_COLUMNS)          # (rows: events, events, firings)
        per_pulse = Columns((('pulse_trigger', np.uint32),))
        for first in range(0, nevents, self.rows_per_chunk):
            nrows = min(self.rows_per_chunk, nevents - first)
            b = bounds[first:first + nrows + 1]
            args = (handle, self.gpu_detector.handle, ctypes.byref(self.tables), nrows, _lib.ptr(b), event.SURFACE_DETECT, ctypes.byref(s),
                    len(gpuphotons.pos), rng, (int(acquisition) + first) & 0xffffffff, float(weight), ctypes.byref(win)) + noise_arg
            naccepted = ctypes.c_uint64(0)
            _lib.check(getattr(lib, 'chroma_daq_count_pulses' + suffix)(*(args + (ctypes.byref(naccepted),))))
            capacity = int(naccepted.value)
            d_offsets = self._room('_pulse_offsets_gpu', nrows + 1)
            d_outside = self._room('_pulse_outside_gpu', 2 * nrows)
            d_row_noise = self._room('_pulse_noise_gpu', nrows)
            arrays = self._room('_pulses_gpu', capacity, kinds(PULSE_COLUMNS))
            npulses = ctypes.c_uint64(0)
            _lib.check(getattr(lib, 'chroma_daq_acquire_pulses' + suffix)(*(args + (capacity, d_offsets.ptr) + tuple(a.ptr for a in arrays) +
                                                                             (d_outside.ptr,) + (() if noise is None else (d_row_noise.ptr,)) +
                                                                             (ctypes.byref(npulses),))))
            npulses = int(npulses.value)
            row_noise = [] if noise is None else [d_row_noise[:nrows].get()]
            offsets = d_offsets[:nrows + 1].get()
            per_row.append([d_outside[:2 * nrows].get().reshape(nrows, 2)] + row_noise)
            pulses.append(offsets, [a[:npulses].get() for a in arrays])
            if trigger is not None:
                got, fired = self._trigger_chunk(win, trigger, nrows, d_offsets, arrays, npulses)
                per_pulse.append([rebase_triggers(got['pulse_trigger'], firings.total)])          # (numbered within the batch)
                firings.append(got['offsets'], columns_of(FIRING_COLUMNS, got))
                hits.append(got['hit_offsets'], columns_of(HIT_COLUMNS, got))
                if digitizer is not None:
                    self._digitize_chunk(win, trigger, digitizer_struct, rng.seed, int(acquisition) + first, nrows, d_offsets, arrays, npulses,
                                         fired, per_hit, found, reducer, keep_traces)
        offsets, columns = pulses.finish()
        rows = per_row.finish()
        result = EventPulses(window, self.nchannels, self.charge_unit, offsets, outside=rows['outside'], noise=rows.get('noise'), **columns)
        if trigger is not None:
            (trigger_offsets, firing_columns), (hit_offsets, hit_columns) = firings.finish(), hits.finish()
            hit_columns.update(firing_columns, **per_pulse.finish())
            result.triggers = EventTriggers(window, trigger, self.nchannels, self.charge_unit, result.offsets, trigger_offsets, hit_offsets=hit_offsets,
                                            pulses=(result.channel, result.bin, result.q_int), **hit_columns)
            if digitizer is not None:
                traces = per_hit.finish()
                if reducer is not None:
                    found_offsets, reduced = found.finish()
                    reduced.update(reducer=reducer, found_offsets=found_offsets, **{name: traces[name] for name in names(REDUCED_COLUMNS)})
                result.triggers = result.triggers.replace(adc=traces.get('adc'), trace_flags=traces['trace_flags'], digitizer=digitizer,
                                                          found=reduced if reducer is not None else None)
        return result
