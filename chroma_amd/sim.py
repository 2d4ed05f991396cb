"""Simulation driver: batches events, propagates them on the GPU and extracts hits.

Reference: chroma/sim.py:21-343 (``Simulation.__init__``, ``_simulate_batch``, ``simulate``, and the PDF entry
points ``create_pdf``, ``eval_pdf``, ``setup_kernel``, ``eval_kernel``).
Out of scope here, as in SURVEY.md section 8: GEANT4 photon generation (``geant4_processes``
is accepted; bare Vertex input and Events without photons or steps need a generator that this package does not provide).
Events whose vertices carry ``steps`` get their photons made on the device (chroma_amd.gpu.steps).  The PDF entry points take
Photons (or Events that carry ``photons_beg``) and run their DAQ acquisitions as GPUDaq(ndaq=K) chunks of at most 64.
"""
import collections
import os
import time
from timeit import default_timer as timer

import numpy as np

from chroma_amd import event, gpu, itertoolset
from chroma_amd.gpu.daq import DaqChain, daq_needs
from chroma_amd.tracks import host_tracks

# simulate()'s names for the stages of a readout (daq_needs), and the readout it resolves once per call for _simulate_batch:
# ``chain`` a DaqChain or None (no daq_window), ``seeder`` a VertexSeeder or None, ``direction`` a DirectionSeeder or None
_DAQ_NAMES = {stage: 'daq_' + stage for stage in ('window', 'trigger', 'noise', 'digitizer', 'reducer', 'seeder', 'direction')}
_Readout = collections.namedtuple('_Readout', 'chain seeder direction')


def cut_batches(iterable, evid_start, photons_per_batch, admit):
    """The events of ``iterable`` in batches: ``admit(ev, evid, index)`` -- the event, its id (on from ``evid_start``) and its index
    in the batch being filled -- refuses the event (raises) or writes on it what its path writes and returns (the event's item in
    the batch, its weight in photons); a batch is closed when its weights reach ``photons_per_batch``, and what is left over
    when the iterable ends is the last one.  Lazy: the iterable is read no further than the batch asked for."""
    total, batch, evid = 0, [], evid_start
    for ev in iterable:
        item, weight = admit(ev, evid, len(batch))
        evid += 1
        total += weight
        batch.append(item)
        if total >= photons_per_batch:
            yield batch
            total, batch = 0, []
    if batch:
        yield batch


def _has_steps(ev):
    return any(getattr(v, 'steps', None) is not None for v in ev.vertices)


# the three ``admit`` of simulate(): events with photons; with steps, weighed by ``expected_photons(segments)``; with neither,
# weighed by ``stepper.expected_photons_at_most(vertices, media)``
def _admit_photons(ev, evid, index):
    ev.id = evid
    ev.nphotons = len(ev.photons_beg)
    ev.photons_beg.evidx[:] = index
    return ev, ev.nphotons


def _admit_stepped(expected_photons):
    def admit(ev, evid, index):
        if ev.photons_beg is not None or not _has_steps(ev):
            raise NotImplementedError('events with steps and events with photons (or with neither) in one simulate() call')
        ev.id = evid
        segments = gpu.steps.segments_from_vertices(ev.vertices, evidx=index)
        return (ev, segments), expected_photons(segments)
    return admit


def _admit_tracked(stepper, media):
    def admit(ev, evid, index):
        if ev.photons_beg is not None or _has_steps(ev):
            raise NotImplementedError('events to be tracked and events with photons or steps in one simulate() call')
        ev.id = evid
        return ev, stepper.expected_photons_at_most(ev.vertices, media)
    return admit


def hits_by_channel(hits):
    """{channel: its hits} of one event's ``hits`` in channel order (as the library hands them over): a channel's hits are one slice."""
    ch = hits.channel
    first = np.flatnonzero(np.concatenate(([True], ch[1:] != ch[:-1]))) if len(ch) else np.zeros(0, np.intp)
    last = np.append(first[1:], len(ch))
    return {c: hits[a:b] for c, a, b in zip(ch[first].tolist(), first.tolist(), last.tolist())}


class _SeederTwins(object):
    """The device twins of simulate()'s seeders and the DirectionSeeder made of what it was given, under one rule: the same
    seeder object as last time -> the same device object."""

    def __init__(self):
        self.direction_of = None             # (what simulate() was given, the DirectionSeeder made of it)
        self._held = {}                      # the class of a seeder -> the device twin made last for one of that class

    def resolve(self, seeder, direction, detector):
        """(the VertexSeeder of ``seeder``, the DirectionSeeder of ``direction`` about it or None)"""
        from chroma_amd.seed import DirectionSeeder, VertexSeeder
        seeder = VertexSeeder.of(seeder, detector)
        if direction is None:
            return seeder, None
        if self.direction_of is None or self.direction_of[0] is not direction or self.direction_of[1].vertex_seeder is not seeder:
            self.direction_of = (direction, DirectionSeeder.of(direction, seeder))
        return seeder, self.direction_of[1]

    def twin(self, seeder, make, *args, **kwargs):
        """``make(*args, seeder, **kwargs)``, made once per seeder object"""
        if type(seeder) not in self._held or self._held[type(seeder)].seeder is not seeder:
            self._held[type(seeder)] = make(*args, seeder, **kwargs)
        return self._held[type(seeder)]


def pick_seed():
    """A seed mixed from the time and the process id (chroma/sim.py:16-19)."""
    return int(time.time()) ^ (os.getpid() << 16) & 2 ** 32 - 1


def _with_outside(stepper, outside):
    """``stepper`` with another ``outside`` row"""
    import copy
    other = copy.copy(stepper)
    other.outside = int(outside)
    return other


class Simulation(object):
    def __init__(self, detector, seed=None, cuda_device=None, particle_tracking=False, photon_tracking=False,
                 geant4_processes=0, nthreads_per_block=64, max_blocks=1024, exact=False, prefetch=True, lanes=1,
                 light_medium=None, stepper=None, daq_seeder=None, daq_direction=None):
        # ``daq_seeder``: what simulate(daq_trigger=...) takes for its ``daq_seeder`` when that is None
        self.daq_seeder = daq_seeder
        # ``daq_direction``: likewise simulate()'s ``daq_direction`` (it needs a ``daq_seeder``, here or there)
        daq_needs(dict(seeder=daq_seeder, direction=daq_direction), _DAQ_NAMES, stages=('direction',))
        self.daq_direction = daq_direction
        # ``light_medium``: the Material whose Cherenkov and scintillation light the steps of Events without photons emit
        # (simulate(); chroma_amd.gpu.steps.LightSource); None: the detector's ``detector_material``; 'located': every segment
        # emits the light of the material it lies in, found on the device in this geometry (chroma_amd.gpu.steps.locate_materials:
        # a LightMedia with a row per material of the detector; a segment outside every solid is in ``detector_material``, or
        # emits nothing when the detector has none)
        self.light_medium = light_medium
        # ``stepper``: a chroma_amd.generator.particles.Stepper, or 'csda' for one with the defaults over the detector's materials
        # (StoppingMedia.from_geometry): simulate() then also takes bare Vertex objects, lists of them, and Events whose vertices
        # have neither photons nor steps -- the vertices are tracked through the geometry on the device (continuous slowing down,
        # no secondaries: chroma_amd.gpu.particles) and emit the light of the medium each step was made in.  None: they are refused.
        if isinstance(stepper, str) and stepper != 'csda':
            raise ValueError("stepper: a Stepper, None or 'csda'")
        self.stepper = stepper               # ('csda': made below, once the detector is flattened)
        self.particle_tracking = bool(particle_tracking)
        self._tracked_media = None           # the LightMedia of the detector's materials, made on first use
        self._particle_base = 0              # particles tracked so far: a particle's random stream is keyed by its global index
        self._light_source = None
        self._outside_row = -1
        self._segment_base = 0               # segments generated so far: a segment's random streams are keyed by its global index
        # ``exact``: propagate with the reference's own traversal loop for every ray (GPUPhotons.propagate(exact=True)):
        # the reference's hit triangle on every ray, several times slower than the default walk
        self.exact = bool(exact)
        # ``prefetch``: simulate() uploads the photons of the NEXT batch (another host thread, the context's second
        # stream, pinned staging buffers) while the current batch propagates; the batches' device arrays come from the
        # library's pool, so after the first two batches nothing is allocated.  The user's iterable is read one batch
        # ahead of the events that are yielded.
        self.prefetch = bool(prefetch)
        # ``lanes`` > 1: simulate() keeps that many batches in flight at once, each on a context of its own (its own streams,
        # queues and working sets; the geometry is uploaded once per lane) driven by a host thread of its own.  On the DEVICE
        # a batch of 1e4-1e6 photons is launch- and latency-bound -- a step under ~1e5 rays lasts as long as its longest ray,
        # the last 8192 photons as long as the longest photon -- and several in flight fill the chip: 2.8 x the photons per
        # second at 1e4 photons per batch, 2 x at 1e6, 1.3 x at 1e7, nothing at 1e8 (device photons, tools/concurrency_probe.py,
        # profiles/r04/concurrency_probe.txt).  END TO END, with host photons in and Python event objects out, the host side
        # of a batch (staging, event objects, hit dictionaries) is most of its time and the lanes share the interpreter: 1.0-1.8 x
        # with four lanes, 0.9-1.3 x with two (profiles/r04/sim_lanes_probe.txt) -- so the default is 1.  Results are those of lanes=1 bit for bit (a photon's random
        # stream is keyed by its global id, handed out in batch order) and are yielded in order.  Not used with photon
        # tracking, keep_photons_beg or run_daq (those take the one-batch-at-a-time loop).
        self.nlanes = max(1, int(lanes))
        self.detector = detector
        self.nthreads_per_block = nthreads_per_block
        self.max_blocks = max_blocks
        # ``photon_tracking``: True -- ev.photon_tracks is a list of Photons, one per photon, built on the host from the per-step
        # copies of GPUPhotons.propagate(track=True) (the reference's way, chroma/sim.py:102-114); 'device' -- the tracks are
        # recorded on the device (GPUPhotons.propagate_tracks) and ev.photon_tracks is a chroma_amd.tracks.PhotonTracks, the same
        # sequence of Photons as slices of one flat array
        if isinstance(photon_tracking, str) and photon_tracking != 'device':
            raise ValueError("photon_tracking: False, True or 'device'")
        self.photon_tracking = photon_tracking
        self.seed = pick_seed() if seed is None else seed
        np.random.seed(self.seed % (2 ** 32))
        self.photon_generator = None      # GEANT4 generation is outside the propagate path

        self.context = gpu.create_cuda_context(cuda_device)
        self._seeders = _SeederTwins()
        if getattr(detector, 'bvh', None) is None:
            from chroma_amd.loader import load_bvh
            detector.flatten()
            detector.bvh = load_bvh(detector)
        make = gpu.GPUDetector if hasattr(detector, 'num_channels') else gpu.GPUGeometry
        packed = None
        if self.nlanes > 1:
            from chroma_amd.gpu.geometry import pack_geometry
            packed = pack_geometry(detector)          # packed once, uploaded once per lane
        self.gpu_geometry = make(detector, packed=packed)
        if isinstance(self.stepper, str):
            from chroma_amd.generator.particles import Stepper, StoppingMedia
            self.stepper = Stepper(StoppingMedia.from_geometry(detector))
        if hasattr(detector, 'num_channels'):
            self.gpu_daq = gpu.GPUDaq(self.gpu_geometry)
        self._gpu_event_daq = None           # the GPUEventDaq of simulate(run_daq=True), made on first use
        self._lanes = [(self.context, self.gpu_geometry)]
        for _ in range(1, self.nlanes):
            ctx = gpu.tools.Context(self.context.device_id)
            with ctx.bound():
                self._lanes.append((ctx, make(detector, packed=packed)))
        packed = None
        self.rng_states = gpu.get_rng_states(self.nthreads_per_block * self.max_blocks, seed=self.seed)
        self.pdf_config = None
        # the PDF entry points' device state, made on first use: GPUPDF, GPUKernelPDF and GPUDaq(ndaq=K) per K
        self._gpu_pdf = self._gpu_pdf_kernel = None
        self._pdf_daqs = {}
        self._pdf_acquisition = 0

    def _upload_batch(self, batch_events, upload=True):
        """The photons of all ``batch_events`` as one GPUPhotons (chroma/sim.py:66-72) + the events' bounds in it.
        With ``upload`` the copies use the context's second stream: safe to run while another batch propagates."""
        # (large events go to their slice of the device arrays directly; many small ones are joined on the host first:
        #  a copy call per array per event would cost more than the concatenation)
        sizes = [len(ev.photons_beg) for ev in batch_events]
        if len(batch_events) == 1 or min(sizes) >= 1_000_000:
            batch_photons = [ev.photons_beg for ev in batch_events]
        else:
            batch_photons = event.Photons.join([ev.photons_beg for ev in batch_events])
        bounds = np.cumsum(np.concatenate([[0], [len(ev.photons_beg) for ev in batch_events]]))
        return gpu.GPUPhotons(batch_photons, copy_triangles=False, copy_weights=False, upload=upload), bounds

    @property
    def _direction_of(self):
        return self._seeders.direction_of

    def _simulate_batch(self, batch_events, keep_photons_beg=False, keep_photons_end=False, keep_hits=True,
                        keep_flat_hits=True, run_daq=False, max_steps=100, verbose=False, uploaded=None, gpu_geometry=None,
                        daq=_Readout(None, None, None)):
        """Propagate the photons of all ``batch_events`` in one go and split the results
        back per event (by evidx).  Yields the events.  ``uploaded``: what _upload_batch returned for them;
        ``gpu_geometry``: the geometry of the lane this batch runs on (default: the simulation's own); ``daq``: the
        _Readout simulate() resolved."""
        t_start = timer()
        geometry = gpu_geometry if gpu_geometry is not None else self.gpu_geometry
        if uploaded is None:
            uploaded = self._upload_batch(batch_events, upload=False)
        gpu_photons, bounds = uploaded
        t_copy = timer()
        want_hits = hasattr(self.detector, 'num_channels') and (keep_hits or keep_flat_hits)
        batch_hits, tracking = self._propagate(gpu_photons, geometry, want_hits, max_steps)
        t_prop = timer()
        if verbose:
            print('GPU copy took %0.2f s' % (t_copy - t_start))
            print('GPU propagate took %0.2f s' % (t_prop - t_copy))

        batch_end = gpu_photons.get() if keep_photons_end else None
        if want_hits and batch_hits is None:
            batch_hits = gpu_photons.get_flat_hits(geometry, sort=True)
        per_event_hits = None if batch_hits is None else self._hits_per_event(batch_hits, len(batch_events))
        acquired = self._read_out(gpu_photons, bounds, daq) if run_daq else None
        for i, (ev, lo, hi) in enumerate(zip(batch_events, bounds[:-1], bounds[1:])):
            if not keep_photons_beg:
                ev.photons_beg = None
            if self.photon_tracking == 'device':
                ev.photon_tracks = tracking.cut(int(lo), int(hi))
            elif self.photon_tracking:
                ev.photon_tracks = host_tracks(tracking[0], tracking[1], lo, hi)
            if keep_photons_end:
                ev.photons_end = batch_end[lo:hi]
            if batch_hits is not None:
                if keep_hits:
                    ev.hits = hits_by_channel(per_event_hits[i])
                if keep_flat_hits:
                    ev.flat_hits = per_event_hits[i]
            if acquired is not None:
                self._attach_readout(ev, i, *acquired)
            elif hasattr(self, 'gpu_daq') and run_daq:
                # (a detector without channels: one acquisition per event, as the reference, chroma/sim.py:128-137)
                self.gpu_daq.begin_acquire()
                self.gpu_daq.acquire(gpu_photons, self.rng_states, start_photon=int(lo), nphotons=int(hi - lo),
                                     nthreads_per_block=self.nthreads_per_block, max_blocks=self.max_blocks)
                ev.channels = self.gpu_daq.end_acquire().get()
            yield ev

    def _propagate(self, gpu_photons, geometry, want_hits, max_steps):
        """The batch's one propagate call: (its flat hits, where the call makes them itself, else None; what tracking gives, else None)."""
        if self.photon_tracking == 'device':
            return None, gpu_photons.propagate_tracks(geometry, self.rng_states, max_steps=max_steps, exact=self.exact)
        if want_hits and not self.photon_tracking:
            # propagate + get_flat_hits as one library call (chroma_propagate_hits): the same set of hits
            return gpu_photons.propagate_hits(geometry, self.rng_states, max_steps=max_steps, exact=self.exact, sort=True), None
        return None, gpu_photons.propagate(geometry, self.rng_states, nthreads_per_block=self.nthreads_per_block, max_blocks=self.max_blocks,
                                           max_steps=max_steps, track=self.photon_tracking, exact=self.exact)

    @staticmethod
    def _hits_per_event(batch_hits, nevents):
        """The hits of each event, and within an event of each channel (hits_by_channel), are SLICES: the library hands the batch's
        hits over in (event, channel) order (chroma_hits_sort: a radix sort and a gather on the device), where the reference masks
        all hits once per event and once per channel (chroma/sim.py:118-123: hits x events + hits x channels element tests --
        2e11 for one 1e8-photon batch on a 29k-channel detector)."""
        if nevents == 1:
            return [batch_hits]
        cuts = np.searchsorted(batch_hits.evidx, np.arange(nevents + 1))
        return [batch_hits[a:b] for a, b in zip(cuts[:-1], cuts[1:])]

    def _read_out(self, gpu_photons, bounds, daq):
        """The DAQ of a batch on a detector with channels (None without them): (the events' channels, their pulses or None, the
        seeds of their firings or None, the directions about those or None)."""
        if not hasattr(self, 'gpu_daq') or self.gpu_geometry.nchannels < 1:
            return None
        # the events' acquisitions as ONE (GPUEventDaq: a row of channels per event, read back sparse), numbered as the
        # reference's one acquisition per event (chroma/sim.py:128-137) numbers them: on from self.gpu_daq's counter
        if self._gpu_event_daq is None:
            self._gpu_event_daq = gpu.GPUEventDaq(self.gpu_geometry)
        acquisition = self.gpu_daq.acquisition
        channels = self._gpu_event_daq.acquire(gpu_photons, self.rng_states, bounds, acquisition=acquisition)
        pulses = vertices = directions = None
        if daq.chain is not None:
            # (under the acquisition numbers of the events' channels: both describe the same photoelectrons)
            pulses = self._gpu_event_daq.acquire_pulses(gpu_photons, self.rng_states, bounds, daq.chain.window, acquisition=acquisition,
                                                        chain=daq.chain)
        self.gpu_daq.acquisition += len(bounds) - 1
        if daq.seeder is not None and pulses is not None and pulses.triggers is not None:
            # every firing of the batch in ONE device call, from what the electronics found where the traces were reduced
            from chroma_amd.gpu.seed import GPUDirectionSeeder, GPUVertexSeeder
            vertex = self._seeders.twin(daq.seeder, GPUVertexSeeder, self.context)
            source = 'reco' if daq.chain.reducer is not None else 'gate'
            if daq.direction is None:
                vertices = pulses.triggers.seed(daq.seeder, source=source, gpu=vertex)
            else:
                # the direction about every seed in a second call, on the rows, positions and bins the first left on the device
                direction = self._seeders.twin(daq.direction, GPUDirectionSeeder, self.context, vertex=vertex)
                vertices, directions = direction.fit_both(vertex, *pulses.triggers.seed_rows(source))
        return channels, pulses, vertices, directions

    @staticmethod
    def _attach_readout(ev, i, channels, pulses, vertices, directions):
        """Event ``i``'s share of what _read_out returned."""
        ev.channels = channels[i]
        if pulses is not None:
            ev.pulses = pulses.event(i)
            if pulses.triggers is not None:
                ev.triggers = pulses.triggers.event(i)
                lo, hi = int(pulses.triggers.offsets[i]), int(pulses.triggers.offsets[i + 1])
                if vertices is not None:
                    ev.triggers.vertices = vertices[lo:hi]
                if directions is not None:
                    ev.triggers.directions = directions[lo:hi]

    def simulate(self, iterable, keep_photons_beg=False, keep_photons_end=False, keep_hits=True,
                 keep_flat_hits=True, run_daq=False, max_steps=1000, photons_per_batch=1000000, evid_start=0, daq_window=None,
                 daq_trigger=None, daq_noise=None, daq_digitizer=None, daq_reducer=None, daq_keep_traces=True, daq_seeder=None,
                 daq_direction=None):
        """Simulate Photons objects (or Events that already carry ``photons_beg``); events are
        batched until ``photons_per_batch`` photons are collected (chroma/sim.py:141-186).

        ``daq_window=(t0, dt, nbins)`` (with ``run_daq=True``, on a detector with channels): besides ``ev.channels`` every event
        gets ``ev.pulses``, the time-binned view of the same photoelectrons (gpu.Pulses: per (channel, bin) npe, charge, earliest
        time and histories; GPUEventDaq.acquire_pulses).  ``daq_trigger`` (with ``daq_window``; a gpu.DaqTrigger or (threshold, width[,
        holdoff, pre, post[, kind]]) in bins): every event also gets ``ev.triggers`` (gpu.Triggers): the firings of a multiplicity
        or photoelectron trigger on those pulses and the channels in each firing's readout gate.  ``daq_noise`` (with ``daq_window``; a
        gpu.DaqNoise, a dark rate in Hz or one per channel): the PMTs' dark counts are drawn into the pulses, flagged
        ``event.DARK_NOISE``, and reach the trigger; ``ev.pulses.noise`` counts them.  ``ev.channels`` does not see them.
        ``daq_digitizer`` (with ``daq_trigger``; a gpu.DaqDigitizer): every gated channel of every firing is read out as a shaped ADC
        trace (``ev.triggers.adc(k)``, ``.trace(k, channel)``, ``.trace_flags``, ``.sample_times(k)``), under the acquisition number
        of the event's channels.  ``daq_reducer`` (with ``daq_digitizer``; a gpu.DaqReducer or (threshold[, lead, lag[, cfd[,
        nbaseline[, min_width]]]])): the traces are reduced on the device to the pulses found in them, with charge and
        constant-fraction time (``ev.triggers.found(k, channel)``, ``.reco(k)``, ``.reco_channels(k)``: an event.Channels of what was
        reconstructed, for Likelihood.set_event); with ``daq_keep_traces=False`` the samples are not read back.  ``daq_seeder`` (with
        ``daq_trigger``; a chroma_amd.seed.VertexSeeder, or a speed in mm/ns or (speed[, spacing_mm[, levels]]) for one over the
        detector's channels; None: the constructor's ``daq_seeder``, which is used only where there is a trigger): every event's
        ``ev.triggers.vertices`` are the ``SeedFits`` of its firings -- a seed vertex and time per firing, fitted on the device for the
        whole batch in one call, from ``reco(k)`` where there is a reducer and from the gate's truth-level hits otherwise.
        ``daq_direction`` (with ``daq_seeder``; a chroma_amd.seed.DirectionSeeder of that seeder, or a cos_c or (cos_c[, sigma_cos[,
        fill[, levels]]]) for a Cherenkov profile; None: the constructor's, used only where there is a seeder): every event's
        ``ev.triggers.directions`` are the ``DirFits`` of its firings about those seeds -- a cone fit per firing, in a second device
        call on the same rows (``chroma_amd.seed.to_vertices`` makes event.Vertex of the two).

        With ``Simulation(prefetch=True)`` (the default) the NEXT batch is taken from ``iterable`` and uploaded by a second
        thread while the current one propagates: the iterable is consumed one batch ahead of the events this generator
        yields.  An iterable whose items share buffers, or depend on results already yielded, needs ``prefetch=False``;
        ``keep_photons_beg=True`` turns the read-ahead off by itself (the reference's loop is lazy, chroma/sim.py:141-186)."""
        given = dict(window=daq_window, trigger=daq_trigger, noise=daq_noise, digitizer=daq_digitizer, reducer=daq_reducer, seeder=daq_seeder)
        daq_needs(given, _DAQ_NAMES, stages=('trigger', 'noise', 'digitizer', 'reducer', 'seeder'))          # (before anything is looked at)
        if daq_seeder is None and daq_trigger is not None:
            daq_seeder = self.daq_seeder
        daq_needs(dict(seeder=daq_seeder, direction=daq_direction), _DAQ_NAMES, stages=('direction',))
        if daq_direction is None and daq_seeder is not None:
            daq_direction = self.daq_direction
        tracked = False
        if isinstance(iterable, event.Photons):
            first, iterable = iterable, [iterable]
        elif isinstance(iterable, event.Vertex) and self.stepper is not None:
            first, iterable = iterable, [iterable]
        else:
            first, iterable = itertoolset.peek(iterable)
        if isinstance(first, event.Photons):
            iterable = (event.Event(photons_beg=x) for x in iterable)
        elif isinstance(first, event.Event):
            if first.photons_beg is None and not self._has_steps(first):
                if self.stepper is None:
                    raise NotImplementedError('events without photons need the GEANT4 generator, which is out of scope')
                tracked = True
        elif self.stepper is not None and self._is_vertices(first):
            iterable = (event.Event(vertices=[x] if isinstance(x, event.Vertex) else list(x)) for x in iterable)
            tracked = True
        else:
            raise NotImplementedError('Vertex input needs the GEANT4 generator, which is out of scope')

        daq = _Readout(None, None, None)
        if daq_window is not None:
            if not run_daq:
                raise ValueError('daq_window needs run_daq=True')
            if not hasattr(self, 'gpu_daq') or self.gpu_geometry.nchannels < 1:
                raise ValueError('daq_window needs a detector with channels')
            chain = DaqChain(daq_window, daq_trigger, daq_noise, daq_digitizer, daq_reducer, daq_keep_traces, nchannels=self.gpu_geometry.nchannels)
            seeders = self._seeders.resolve(daq_seeder, daq_direction, self.detector) if daq_seeder is not None else (None, None)
            daq = _Readout(chain, *seeders)
        kwargs = dict(keep_photons_beg=keep_photons_beg, keep_photons_end=keep_photons_end, keep_hits=keep_hits,
                      keep_flat_hits=keep_flat_hits, run_daq=run_daq, max_steps=max_steps, daq=daq)
        if tracked:
            yield from self._simulate_tracked(iterable, photons_per_batch, evid_start, kwargs)
            return
        if isinstance(first, event.Event) and first.photons_beg is None:
            yield from self._simulate_stepped(iterable, photons_per_batch, evid_start, kwargs)
            return
        batches = cut_batches(iterable, evid_start, photons_per_batch, _admit_photons)
        # (read-ahead contract: with prefetch the iterable is pulled one batch ahead of the events being yielded, and `evidx` is
        #  written into the photons of that next batch early; a generator that reuses its buffers, or a caller who wants
        #  `photons_beg` back untouched, gets the reference's lazy loop instead)
        if self.nlanes > 1 and not (self.photon_tracking or keep_photons_beg or run_daq):
            yield from self._simulate_lanes(batches, kwargs)
            return
        if not self.prefetch or self.photon_tracking or keep_photons_beg:
            for batch in batches:
                yield from self._simulate_batch(batch, **kwargs)
            return
        # one batch ahead: while batch k propagates (the library call releases the GIL), a second thread stages and
        # uploads batch k + 1 on the context's second stream
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=1) as pool:
            cur = next(batches, None)
            fut = pool.submit(self._upload_batch, cur) if cur is not None else None
            while cur is not None:
                uploaded = fut.result()
                nxt = next(batches, None)
                fut = pool.submit(self._upload_batch, nxt) if nxt is not None else None
                yield from self._simulate_batch(cur, uploaded=uploaded, **kwargs)
                uploaded = None
                cur = nxt

    # ---- events that carry steps instead of photons ------------------------------------------------------------------
    _has_steps = staticmethod(_has_steps)

    @property
    def light_source(self):
        """The LightSource of ``light_medium`` (or of the detector's ``detector_material``), made on first use; with
        ``light_medium='located'`` the LightMedia of the detector's materials."""
        if self._light_source is None and isinstance(self.light_medium, str):
            if self.light_medium != 'located':
                raise ValueError("light_medium: a Material, None or 'located'")
            materials = list(self.detector.unique_materials)
            outside = getattr(self.detector, 'detector_material', None)
            if outside is not None:
                rows = [m for m, have in enumerate(materials) if have is outside]
                if not rows:
                    materials.append(outside)          # (a row of its own behind the geometry's: no triangle names it)
                self._outside_row = rows[0] if rows else len(materials) - 1
            self._light_source = gpu.steps.LightMedia(materials)
        if self._light_source is None:
            medium = self.light_medium if self.light_medium is not None else getattr(self.detector, 'detector_material', None)
            if medium is None:
                raise ValueError('events with steps need a medium: Simulation(light_medium=...) or the detector\'s detector_material')
            self._light_source = gpu.steps.LightSource(medium)
        return self._light_source

    def _simulate_stepped(self, iterable, photons_per_batch, evid_start, kwargs):
        """Events without ``photons_beg`` whose vertices carry ``steps``: the photons of a batch are generated on the device
        (chroma_amd.gpu.steps.generate_photons, seed ``self.seed``) and propagated where they are.  Events are batched by the
        photons their steps are EXPECTED to emit; the segments of the events are numbered on in iterable order from one
        simulate() call to the next, so the photons do not depend on the batching.  ``photons_beg`` is fetched only with
        ``keep_photons_beg``.

        With ``light_medium='located'`` the medium of a segment is not known before its batch is on the device, and the
        batches have to be cut before anything is drawn; so an event counts with what its segments would emit each in the
        medium it emits MOST in (LightMedia.expected_at_most).  That is an upper bound of what it is expected to emit: a
        batch is closed no later than the true media would close it, so it never grows beyond what ``photons_per_batch``
        allows for a single medium, and may hold fewer photons."""
        source = self.light_source
        located = isinstance(source, gpu.steps.LightMedia)
        expected_photons = source.expected_at_most if located else source.expected_photons

        for batch in cut_batches(iterable, evid_start, photons_per_batch, _admit_stepped(expected_photons)):
            segments = gpu.steps.Segments.join([s for _, s in batch], segment_base=self._segment_base)
            self._segment_base += len(segments)
            where = dict(gpu_geometry=self.gpu_geometry, outside=self._outside_row) if located else {}
            gpu_photons, offsets = gpu.steps.generate_photons(segments, source, self.seed, ctx=self.context, return_offsets=True, **where)
            cuts = 2 * np.cumsum([0] + [len(s) for _, s in batch])
            yield from self._simulate_generated([ev for ev, _ in batch], gpu_photons, offsets[cuts].astype(np.int64), kwargs)

    def _simulate_generated(self, events, gpu_photons, bounds, kwargs):
        """The tail of a batch whose photons were made on the device: event k's are ``bounds[k]:bounds[k + 1]`` of ``gpu_photons``."""
        photons_beg = gpu_photons.get() if kwargs['keep_photons_beg'] else None
        for ev, lo, hi in zip(events, bounds[:-1], bounds[1:]):
            ev.nphotons = int(hi - lo)
            if photons_beg is not None:
                ev.photons_beg = photons_beg[int(lo):int(hi)]
        yield from self._simulate_batch(events, uploaded=(gpu_photons, bounds), **kwargs)

    # ---- vertices that carry nothing: tracked on the device (Simulation(stepper=...)) ---------------------------------
    @staticmethod
    def _is_vertices(x):
        return isinstance(x, event.Vertex) or (isinstance(x, (list, tuple)) and len(x) > 0 and all(isinstance(v, event.Vertex) for v in x))

    def _simulate_tracked(self, iterable, photons_per_batch, evid_start, kwargs):
        """Events whose vertices have neither photons nor steps.  A batch stays in device memory from its vertices to its hits:
        the vertices are tracked through the geometry (chroma_amd.gpu.particles.track_segments; a particle with no triangle
        ahead is in ``stepper.outside`` or, when that is -1, in the detector's ``detector_material`` if it is one of the
        geometry's materials), the segments and the medium each was made in go to the light source (a LightMedia of the
        detector's materials) where they are, and the photons are propagated where they are generated.  Particles and
        segments are numbered on in iterable order from one simulate() call to the next, so nothing depends on the batching.

        Batches are cut before anything is tracked, by ``Stepper.expected_photons_at_most``: every particle loses all its
        kinetic energy at the smallest stopping power of its species, radiating at beta = 1 in the brightest medium all the
        way.  That over-estimates, so a batch is closed early rather than late.  With ``particle_tracking=True`` the points
        are read back and the events' vertices are copies that carry them as ``steps``."""
        stepper = self.stepper
        if self._tracked_media is None:
            self._tracked_media = gpu.steps.LightMedia.from_geometry(self.detector)
        media = self._tracked_media
        outside = stepper.outside
        if outside < 0:
            material = getattr(self.detector, 'detector_material', None)
            outside = stepper.media.index(material) if material is not None else -1
        options_stepper = stepper if outside == stepper.outside else _with_outside(stepper, outside)

        for events in cut_batches(iterable, evid_start, photons_per_batch, _admit_tracked(stepper, media)):
            vertices = [v for ev in events for v in ev.vertices]
            evidx = np.array([i for i, ev in enumerate(events) for _ in ev.vertices], dtype=np.uint32)
            made = gpu.particles.track_segments(vertices, options_stepper, self.seed, gpu_geometry=self.gpu_geometry, ctx=self.context,
                                                particle_base=self._particle_base, evidx=evidx, segment_base=self._segment_base,
                                                return_tracks=self.particle_tracking)
            segments = made[0] if self.particle_tracking else made
            self._particle_base += len(vertices)
            self._segment_base += len(segments)
            gpu_photons, offsets = gpu.steps.generate_photons(segments, media, self.seed, ctx=self.context, return_offsets=True)
            if self.particle_tracking:
                stepped = iter(made[1])
                for ev in events:
                    ev.vertices = [next(stepped) for _ in ev.vertices]
            # (segments, and so photons, are in event order: an event's bounds from its segments' -- their event indices and the
            #  scanned counts are all that is read back, 12 bytes a segment)
            cuts = np.searchsorted(segments.arrays['evidx'].get()[:len(segments)], np.arange(len(events) + 1))
            yield from self._simulate_generated(events, gpu_photons, offsets[2 * cuts].astype(np.int64), kwargs)

    def _simulate_lanes(self, batches, kwargs):
        """``lanes`` batches in flight at once, each on its own context from its own host thread (the library calls
        release the GIL); events come back in the order of the iterable.  The photon-id block of a batch (its random
        streams) is reserved HERE, in batch order, so the results are those of the one-batch-at-a-time loop."""
        from collections import deque
        from concurrent.futures import ThreadPoolExecutor

        def work(lane, batch, rng_base):
            ctx, geometry = self._lanes[lane]
            with ctx.bound():
                uploaded = self._upload_batch(batch, upload=False)
                uploaded[0]._rng_base, uploaded[0]._rng_owner = rng_base, self.rng_states
                return list(self._simulate_batch(batch, uploaded=uploaded, gpu_geometry=geometry, **kwargs))

        with ThreadPoolExecutor(max_workers=self.nlanes) as pool:
            free, pending = deque(range(self.nlanes)), deque()
            for batch in batches:
                if not free:
                    lane, fut = pending.popleft()
                    events = fut.result()
                    free.append(lane)
                    yield from events
                lane = free.popleft()
                base = self.rng_states.reserve(sum(len(ev.photons_beg) for ev in batch))
                pending.append((lane, pool.submit(work, lane, batch, base)))
            while pending:
                lane, fut = pending.popleft()
                yield from fut.result()

    # ---- PDFs and likelihood terms (chroma/sim.py:188-343) ----------------------------------------------------------
    @property
    def gpu_pdf(self):
        if self._gpu_pdf is None:
            self._gpu_pdf = gpu.GPUPDF(self.context)
        return self._gpu_pdf

    @property
    def gpu_pdf_kernel(self):
        if self._gpu_pdf_kernel is None:
            self._gpu_pdf_kernel = gpu.GPUKernelPDF(self.context)
        return self._gpu_pdf_kernel

    @staticmethod
    def _photon_sets(iterable):
        """The Photons of each item of ``iterable`` (Photons, or Events that carry photons_beg), as ``simulate`` takes them."""
        if isinstance(iterable, event.Photons):
            iterable = [iterable]
        first, iterable = itertoolset.peek(iterable)
        if isinstance(first, event.Photons):
            return iterable
        if isinstance(first, event.Event):
            if first.photons_beg is None:
                raise NotImplementedError('events without photons need the GEANT4 generator, which is out of scope')
            return (ev.photons_beg for ev in iterable)
        raise NotImplementedError('Vertex input needs the GEANT4 generator, which is out of scope')

    def _daq_chunks(self, ndaq):
        """GPUDaq objects for ``ndaq`` acquisitions of one photon set, at most 64 copies each."""
        if ndaq < 1:
            raise ValueError('ndaq must be at least 1')
        for first in range(0, ndaq, 64):
            k = min(64, ndaq - first)
            if k not in self._pdf_daqs:
                self._pdf_daqs[k] = gpu.GPUDaq(self.gpu_geometry, ndaq=k)
            yield self._pdf_daqs[k]

    def _acquire(self, daq, sources):
        """One acquisition (``daq.ndaq`` copies) of the (photons, weight) ``sources``.  The PDF entry points' GPUDaq
        objects share one acquisition counter, so two of them never draw the same random numbers for one photon."""
        daq.acquisition = self._pdf_acquisition
        daq.begin_acquire()
        for photons, weight in sources:
            daq.acquire(photons, self.rng_states, nthreads_per_block=self.nthreads_per_block, max_blocks=self.max_blocks,
                        weight=weight)
        self._pdf_acquisition = daq.acquisition
        return daq.end_acquire()

    def create_pdf(self, iterable, tbins, trange, qbins, qrange, nreps=1):
        """Returns tuple: 1D array of channel hit counts, 3D array of (channel, time, charge) pdfs."""
        photon_sets = self._photon_sets(iterable)
        pdf_config = (tbins, trange, qbins, qrange)
        if pdf_config != self.pdf_config:
            self.pdf_config = pdf_config
            self.gpu_pdf.setup_pdf(self.detector.num_channels(), tbins, trange, qbins, qrange)
        else:
            self.gpu_pdf.clear_pdf()
        if nreps > 1:
            photon_sets = (p for p in photon_sets for _ in range(nreps))
        daq = next(self._daq_chunks(1))
        for photons in photon_sets:
            gpu_photons = gpu.GPUPhotons(photons)
            gpu_photons.propagate(self.gpu_geometry, self.rng_states, nthreads_per_block=self.nthreads_per_block,
                                  max_blocks=self.max_blocks)
            self.gpu_pdf.add_hits_to_pdf(self._acquire(daq, [(gpu_photons, 1.0)]))
        return self.gpu_pdf.get_pdfs()

    def eval_pdf(self, event_channels, iterable, min_twidth, trange, min_qwidth, qrange, min_bin_content=100, nreps=1,
                 ndaq=1, nscatter=1, time_only=True):
        """Returns tuple: 1D array of channel hit counts, 1D array of PDF probability densities, 1D array of their
        uncertainties.  Each photon set is propagated ``nreps`` times without scattering and ``nreps * nscatter`` times
        scattering at the first step (weighted photons, chroma/sim.py:236-294); each of those runs through exactly
        ``ndaq`` DAQ acquisitions, in chunks of at most 64 copies and one accumulate call per chunk."""
        self.gpu_pdf.setup_pdf_eval(event_channels.hit, event_channels.t, event_channels.q, min_twidth, trange,
                                    min_qwidth, qrange, min_bin_content=min_bin_content, time_only=True)
        for photons in self._photon_sets(iterable):
            gpu_photons_no_scatter = gpu.GPUPhotons(photons, ncopies=nreps)
            gpu_photons_scatter = gpu.GPUPhotons(photons, ncopies=nreps * nscatter)
            gpu_photons_no_scatter.propagate(self.gpu_geometry, self.rng_states, nthreads_per_block=self.nthreads_per_block,
                                             max_blocks=self.max_blocks, use_weights=True, scatter_first=-1, max_steps=10)
            gpu_photons_scatter.propagate(self.gpu_geometry, self.rng_states, nthreads_per_block=self.nthreads_per_block,
                                          max_blocks=self.max_blocks, use_weights=True, scatter_first=1, max_steps=5)
            nphotons = gpu_photons_no_scatter.true_nphotons
            for i in range(nreps):
                no_scatter = gpu_photons_no_scatter.select(event.SURFACE_DETECT, start_photon=i * nphotons, nphotons=nphotons)
                if len(no_scatter) == 0:
                    continue
                sources = [(no_scatter, 1.0)]
                sources += [(gpu_photons_scatter.select(event.SURFACE_DETECT, start_photon=(nscatter * i + j) * nphotons,
                                                        nphotons=nphotons), 1.0 / nscatter) for j in range(nscatter)]
                for daq in self._daq_chunks(ndaq):
                    self.gpu_pdf.accumulate_pdf_eval(self._acquire(daq, sources))
        return self.gpu_pdf.get_pdf_eval()

    def _accumulate_copies(self, iterable, nreps, ndaq, accumulate):
        for photons in self._photon_sets(iterable):
            gpu_photons = gpu.GPUPhotons(photons, ncopies=nreps)
            gpu_photons.propagate(self.gpu_geometry, self.rng_states, nthreads_per_block=self.nthreads_per_block,
                                  max_blocks=self.max_blocks)
            for gpu_photon_slice in gpu_photons.iterate_copies():
                for daq in self._daq_chunks(ndaq):
                    accumulate(self._acquire(daq, [(gpu_photon_slice, 1.0)]))

    def setup_kernel(self, event_channels, bandwidth_iterable, trange, qrange, nreps=1, ndaq=1, time_only=True,
                     scale_factor=1.0):
        """Call this before eval_kernel(): sets up the event information and computes the kernel bandwidths."""
        self.gpu_pdf_kernel.setup_moments(len(event_channels.hit), trange, qrange, time_only=time_only)
        self._accumulate_copies(bandwidth_iterable, nreps, ndaq, self.gpu_pdf_kernel.accumulate_moments)
        self.gpu_pdf_kernel.compute_bandwidth(event_channels.hit, event_channels.t, event_channels.q,
                                              scale_factor=scale_factor)

    def eval_kernel(self, event_channels, kernel_iterable, trange, qrange, nreps=1, ndaq=1, naverage=1, time_only=True):
        """Returns tuple: 1D array of channel hit counts, 1D array of PDF probability densities, zeros."""
        self.gpu_pdf_kernel.setup_kernel(event_channels.hit, event_channels.t, event_channels.q)
        self._accumulate_copies(kernel_iterable, nreps, ndaq, self.gpu_pdf_kernel.accumulate_kernel)
        return self.gpu_pdf_kernel.get_kernel_eval()

    def __del__(self):
        try:
            for ctx, geometry in self._lanes[1:]:
                ctx.synchronize()
            self.context.pop()
        except Exception:
            pass
