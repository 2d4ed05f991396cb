"""The digitiser of the time-binned DAQ on the GPU -- chroma_daq_digitize_gates (k_daq_digitize), GPUEventDaq.acquire_pulses(
digitizer=...) and Simulation.simulate(daq_digitizer=...) over it -- bit for bit on the brute-force restatement of
tests/test_daq_digitize_host.py, on that module's pulse sets and digitisers (uploaded as they are: the digitiser is a function of
the pulse, trigger and hit arrays) and on what the library itself acquires.  Every output array is longer than what the call may
write and pre-filled with a sentinel, which the words beyond must still hold.
"""
import ctypes

import numpy as np
import pytest

from chroma_amd import event
from test_gpu_photon_arrays import geos, host_geos, gpu, upload, DAQ_BASE      # noqa: F401
from test_gpu_daq_events import BASE, WEIGHT
from test_daq_pulses_host import restated, W_ALL, SEED as PHOTON_SEED          # noqa: F401
from test_daq_trigger_host import cases, brute, brute_of, bits
from test_gpu_daq_trigger import more_sets
from test_daq_digitize_host import (digitisers, brute_adc, brute_traces, handmade, handmade_results, call_arguments, ORDER, SENTINEL16, SENTINEL32, ERR_INVALID,
                                    SEED, ACQUISITION, Digitiser, refusals, assert_traces, garbage_case)

pytestmark = pytest.mark.gpu


def device_rc(gpu, ps, trig, want, dig, seed=SEED, acquisition=ACQUISITION, first_hit=0, nhits_call=None, capacity=None, guard=8, change=None, struct_change=None):
    """chroma_daq_digitize_gates into sentinel-filled device arrays `guard` entries longer than the slice needs; (rc, adc, flags)."""
    from chroma_amd import _lib
    from chroma_amd.gpu.tools import to_gpu
    ctx = gpu.get_context()
    G = trig[3] + trig[4]
    nhits = len(want['hit_channel'])
    nhits_call = nhits - first_hit if nhits_call is None else nhits_call
    ntraces = max(0, min(nhits_call, nhits))
    room = ntraces * min(G, 65536)
    adc = to_gpu(np.full(room + guard, SENTINEL16, dtype=np.uint16))
    flags = to_gpu(np.full(ntraces + guard, SENTINEL32, dtype=np.uint32))
    v = call_arguments(ps, trig, want, dig.struct(**(struct_change or {})), seed, acquisition, first_hit, nhits_call, room if capacity is None else capacity,
                       adc, flags, change)
    keep = []
    args = [ctx.handle]
    for k in ORDER:
        a = v[k]
        if isinstance(a, np.ndarray):
            keep.append(to_gpu(a) if len(a) else None)
            a = keep[-1].ptr if len(a) else None
        elif isinstance(a, ctypes.Structure):
            a = ctypes.byref(a)
        elif hasattr(a, 'ptr'):
            a = a.ptr
        args.append(a)
    rc = ctx._lib.chroma_daq_digitize_gates(*args)
    ctx.synchronize()
    return rc, adc.get(), flags.get()


def run(gpu, ps, trig, want, dig, want_adc, want_flags, what, **kw):
    from chroma_amd import _lib
    rc, adc, flags = device_rc(gpu, ps, trig, want, dig, **kw)
    _lib.check(rc)
    assert_traces(adc, flags, want_adc, want_flags, what)


# ---- 1. the call is the restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', range(5))
def test_the_call_is_the_restatement_on_the_trigger_sets(gpu, which):
    dig = digitisers()[which]
    for index, (name, ps, trig) in enumerate(cases()):
        want_adc, want_flags = brute_traces(index, which)
        run(gpu, ps, trig, brute(index, 'nhit'), dig, want_adc, want_flags, '%s, %s' % (name, dig.name))


def test_the_call_is_the_restatement_on_the_handmade_sets(gpu):
    for (name, ps, trig, dig), (want, want_adc, want_flags) in zip(handmade(), handmade_results()):
        run(gpu, ps, trig, want, dig, want_adc, want_flags, name)


def test_300_rows_of_one_bin_where_the_row_changes_at_every_trace(gpu):
    name, ps, trig = next(more_sets())
    assert ps.nrows == 300 and ps.nbins == 1
    want = brute_of(ps, 'nhit', *trig)
    per_row = np.diff(want['trig_offsets'].astype(np.int64))
    assert per_row.max() == 1 and per_row.min() == 0 and per_row.sum() > 64 and len(want['hit_channel']) > 2 * per_row.sum()
    dig = Digitiser('two taps, noise', [1 << 20, 1 << 19], 31, 50, 12, 2.0)
    want_adc, want_flags = brute_adc(ps, trig, want, dig)
    run(gpu, ps, trig, want, dig, want_adc, want_flags, name)


# ---- 2. slices and capacities ---------------------------------------------------------------------------------------------------------------
def test_a_slice_is_that_part_of_the_whole(gpu):
    index, which = 1, 4
    name, ps, trig = cases()[index]
    want = brute(index, 'nhit')
    want_adc, want_flags = brute_traces(index, which)
    nhits = len(want_adc)
    inside = int(want['hit_offsets'][1]) + 1          # (inside the hits of the second trigger)
    assert want['hit_offsets'][1] < inside < want['hit_offsets'][2]
    for first, n in ((inside, 7), (nhits - 1, 1), (3, nhits - 3), (0, 5)):
        run(gpu, ps, trig, want, digitisers()[which], want_adc[first:first + n], want_flags[first:first + n], 'hits [%d, %d)' % (first, first + n),
            first_hit=first, nhits_call=n)


def test_no_hits_in_the_call_is_ok_and_writes_nothing(gpu):
    name, ps, trig = cases()[0]
    want = brute(0, 'nhit')
    for first in (0, 2, len(want['hit_channel'])):
        for change in (None, dict(adc=None, flags=None)):
            rc, adc, flags = device_rc(gpu, ps, trig, want, digitisers()[1], first_hit=first, nhits_call=0, change=change)
            assert rc == 0 and (adc == SENTINEL16).all() and (flags == SENTINEL32).all()


def test_what_the_header_refuses_is_refused_before_anything_is_launched(gpu):
    """Among them a capacity one sample short: nothing is written."""
    name, ps, trig = cases()[0]
    want = brute(0, 'nhit')
    for what, kw in refusals():
        kw = dict(kw)
        kw.pop('keep', None)
        rc, adc, flags = device_rc(gpu, ps, trig, want, digitisers()[1], **kw)
        assert rc == ERR_INVALID, what
        assert (adc == SENTINEL16).all() and (flags == SENTINEL32).all(), what
    rc, adc, flags = device_rc(gpu, ps, trig, want, digitisers()[1], change=dict(nrows=ps.nrows), capacity=len(want['hit_channel']) * 6)
    assert rc == 0 and not (adc[:-8] == SENTINEL16).all()


# ---- 3. entries that count for nothing ----------------------------------------------------------------------------------------------------------
def test_a_channel_outside_the_detector_and_a_trigger_in_no_row_have_no_signal(gpu):
    """test_daq_digitize_host.garbage_case: every index the kernel forms from these arrays stays within the arrays of this test; only
    values are compared."""
    ps, trig, dig, want, want_adc, want_flags = garbage_case()
    run(gpu, ps, trig, want, dig, want_adc, want_flags, 'entries that count for nothing')


# ---- 4. GPUEventDaq.acquire_pulses(digitizer=...) ---------------------------------------------------------------------------------------------------
def test_acquire_pulses_with_a_digitiser_is_the_host_twin_whatever_the_chunking(gpu, geos, restated):
    from chroma_amd import _lib
    geo = geos['tiny']
    rows, bounds, acc = restated('tiny', 'many')
    nrows = len(bounds) - 1
    dev = upload(rows)
    trigger = gpu.DaqTrigger(1, 4, 8, 2, 6)
    digitizer = gpu.DaqDigitizer.biexponential(40.0, 0.5, 2.0, W_ALL[1], bits=12, pedestal=200, noise_sigma=1.5)
    noise = gpu.DaqNoise(2e6)
    results = {}
    for rows_per_chunk in (7, None):
        event_daq = gpu.GPUEventDaq(geo.gg) if rows_per_chunk is None else gpu.GPUEventDaq(geo.gg, max_entries=7 * geo.nchannels + geo.nchannels - 1)
        assert event_daq.rows_per_chunk == (rows_per_chunk or event_daq.rows_per_chunk) and (rows_per_chunk or event_daq.rows_per_chunk >= nrows)
        rng = _lib.Rng(PHOTON_SEED, DAQ_BASE)
        if rows_per_chunk:
            event_daq.max_entries = 40          # (the samples of one digitiser call: slices of 5 hits)
        plain = event_daq.acquire_pulses(dev, rng, bounds, W_ALL, acquisition=BASE, weight=WEIGHT, trigger=trigger, noise=noise)
        pulses = event_daq.acquire_pulses(dev, rng, bounds, W_ALL, acquisition=BASE, weight=WEIGHT, trigger=trigger, noise=noise, digitizer=digitizer)
        for name in ('offsets', 'channel', 'bin', 'npe', 'q_int', 't_first', 'flags', 'q', 'noise'):
            assert np.array_equal(bits(getattr(pulses, name)), bits(getattr(plain, name))), name
        t, p = pulses.triggers, plain.triggers
        for name in ('offsets', 'bin', 'sum', 'hit_offsets', 'hit_channel', 'hit_npe', 'hit_q_int', 'hit_t_first', 'hit_flags', 'pulse_trigger'):
            assert np.array_equal(bits(getattr(t, name)), bits(getattr(p, name))), name
        assert p.adc is None and p.trace_flags is None and t.digitizer == digitizer
        assert t.adc.dtype == np.uint16 and t.adc.shape == (len(t.hit_channel), 8) and t.trace_flags.dtype == np.uint32 and len(t.trace_flags) == len(t.adc)
        if rows_per_chunk:          # (several slices of hits per chunk, too)
            assert event_daq.max_entries // 8 == 5 < np.diff(t.hit_offsets[t.offsets[::7]]).max()
        for offline in (t.digitize(digitizer, seed=PHOTON_SEED, acquisition=BASE), pulses.trigger(trigger).digitize(digitizer, seed=PHOTON_SEED, acquisition=BASE)):
            assert np.array_equal(offline.adc, t.adc) and np.array_equal(offline.trace_flags, t.trace_flags), '%s rows per chunk against the host' % rows_per_chunk
        results[rows_per_chunk] = t
    assert np.array_equal(results[7].adc, results[None].adc) and np.array_equal(results[7].trace_flags, results[None].trace_flags)
    adc = results[7].adc
    assert len(adc) > 100 and adc.max() > 200 + 32 and len(np.unique(adc)) > 20          # (beyond pedestal and noise)
    with pytest.raises(ValueError):
        event_daq.acquire_pulses(dev, rng, bounds, W_ALL, digitizer=digitizer)
    with pytest.raises(ValueError, match='high word'):
        event_daq.acquire_pulses(dev, _lib.Rng(PHOTON_SEED, (0xffffffff << 32) - 5), bounds, W_ALL, trigger=trigger, digitizer=digitizer)


def test_one_event_daq_takes_a_long_gate_and_then_a_short_one_with_more_traces_per_slice(gpu, geos, restated):
    """The buffers of the samples and of the flag words are kept on the GPUEventDaq and grown each on its own.  640 samples per call:
    ten traces of 64 samples, then eighty of 8 -- as many samples, eight times the flag words -- and back; every result is the host
    twin's of the same pulses and triggers."""
    from chroma_amd import _lib
    geo = geos['tiny']
    rows, bounds, acc = restated('tiny', 'many')
    dev = upload(rows)
    digitizer = gpu.DaqDigitizer.biexponential(40.0, 0.5, 2.0, W_ALL[1], bits=12, pedestal=200, noise_sigma=1.5)
    event_daq = gpu.GPUEventDaq(geo.gg)
    event_daq.max_entries = 640
    rng = _lib.Rng(PHOTON_SEED, DAQ_BASE)
    for trigger, per_slice in ((gpu.DaqTrigger(1, 4, 64, 8, 56), 10), (gpu.DaqTrigger(1, 4, 8, 2, 6), 80), (gpu.DaqTrigger(1, 4, 64, 8, 56), 10)):
        G = trigger.pre + trigger.post
        assert event_daq.max_entries // G == per_slice
        pulses = event_daq.acquire_pulses(dev, rng, bounds, W_ALL, acquisition=BASE, weight=WEIGHT, trigger=trigger, digitizer=digitizer)
        t = pulses.triggers
        assert len(t.hit_channel) > 2 * per_slice and t.adc.shape == (len(t.hit_channel), G)          # (several slices, the first ones full)
        assert len(event_daq._adc_gpu) >= per_slice * G and len(event_daq._trace_flags_gpu) >= per_slice
        offline = t.digitize(digitizer, seed=PHOTON_SEED, acquisition=BASE)
        assert np.array_equal(offline.adc, t.adc) and np.array_equal(offline.trace_flags, t.trace_flags), 'a gate of %d samples' % G
    assert len(event_daq._adc_gpu) == 640 and len(event_daq._trace_flags_gpu) == 80


# ---- 5. through Simulation and chroma-sim ------------------------------------------------------------------------------------------------------------
def test_simulation_gives_every_event_the_traces_of_the_offline_path_and_nothing_else_changes(gpu, tiny_geometry, tmp_path):
    from conftest import bomb
    from chroma_amd import cli
    from chroma_amd.gpu import tools
    from chroma_amd.sim import Simulation
    previous = tools._current
    window = (-8.0, 0.5, 512)
    trigger = gpu.DaqTrigger(2, 16, 64, 8, 40)
    digitizer = gpu.DaqDigitizer.biexponential(30.0, 1.0, 6.0, 0.5, bits=12, pedestal=150, noise_sigma=2.0)
    sizes = [400, 1, 3000, 64]
    try:
        runs = {}
        for digitised in (False, True):
            batch = [bomb(n, seed=300 + k) for k, n in enumerate(sizes)]
            batch.insert(2, event.Photons())
            sim = Simulation(tiny_geometry, seed=21)
            seed = sim.rng_states.seed
            kw = dict(daq_digitizer=digitizer) if digitised else {}
            runs[digitised] = list(sim.simulate(batch, run_daq=True, max_steps=100, daq_window=window, daq_trigger=trigger, **kw))
            if digitised:
                with pytest.raises(ValueError):
                    list(sim.simulate(batch, run_daq=True, daq_window=window, daq_digitizer=digitizer))
                with pytest.raises(ValueError):
                    list(sim.simulate(batch, run_daq=True, daq_window=window, daq_trigger=(2, 16, 70000, 30000, 40000), daq_digitizer=digitizer))
            del sim
        ntraces = 0
        for i, (plain, ev) in enumerate(zip(runs[False], runs[True])):
            assert plain.triggers.traces is None and isinstance(ev.triggers, gpu.Triggers)
            for name in ('t', 'q', 'flags', 'hit'):
                assert np.array_equal(bits(getattr(ev.channels, name)), bits(getattr(plain.channels, name))), 'event %d: channels.%s' % (ev.id, name)
            for name in ('channel', 'bin', 'npe', 'q_int', 't_first', 'flags'):
                assert np.array_equal(bits(getattr(ev.pulses, name)), bits(getattr(plain.pulses, name))), 'event %d: pulses.%s' % (ev.id, name)
            for name in ('bin', 'sum', 'hit_offsets', 'hit_channel', 'hit_npe', 'hit_q_int', 'hit_t_first', 'hit_flags', 'pulse_trigger'):
                assert np.array_equal(bits(getattr(ev.triggers, name)), bits(getattr(plain.triggers, name))), 'event %d: triggers.%s' % (ev.id, name)
            # ev.triggers' traces are ev.pulses triggered and digitised on the host, as acquisition i
            p = ev.pulses
            alone = gpu.EventPulses(p.window, p.nchannels, ev.triggers.charge_unit, np.array([0, len(p)], dtype=np.int64), p.channel, p.bin, p.npe, p.q_int,
                                    p.t_first, p.flags, outside=np.zeros((1, 2), dtype=np.uint32))
            want = alone.trigger(trigger).digitize(digitizer, seed=seed, acquisition=i).event(0)
            t = ev.triggers
            assert t.traces.dtype == np.uint16 and t.traces.shape == (len(t.hit_channel), 48)
            assert np.array_equal(t.traces, want.traces) and np.array_equal(t.trace_flags, want.trace_flags), 'event %d' % ev.id
            for k in range(len(t)):
                channels, traces = t.adc(k)
                assert np.array_equal(channels, t.sparse(k)[0]) and np.array_equal(t.trace(k, channels[0]), traces[0])
                assert np.array_equal(t.sample_times(k), window[0] + window[1] * (int(t.bin[k]) - 8 + np.arange(48, dtype=np.float64)))
            ntraces += len(t.traces)
        assert ntraces >= 3 and max(int(ev.triggers.traces.max()) for ev in runs[True] if len(ev.triggers.traces)) > 150 + 32
        # chroma-sim --daq-digitize: the trace arrays beside those of --daq-trigger
        files = {}
        for flag in ('trigger', 'digitize'):
            files[flag] = str(tmp_path / (flag + '.npz'))
            argv = ['@chroma_amd.demo.tiny', '-n', '2', '--nphotons', '900', '-s', '4', '--max-steps', '100', '-o', files[flag], '--daq-window=-8,0.5,512',
                    '--daq-trigger', '2,16,64,8,40']
            assert cli.main(argv + (['--daq-digitize', '30,1,6,12,150,2'] if flag == 'digitize' else [])) == 0
        triggered, digitised = np.load(files['trigger']), np.load(files['digitize'])
        assert sorted(digitised.files) == sorted(triggered.files + ['ev%d/%s' % (k, name) for k in range(2) for name in ('trigger_adc', 'trigger_trace_flags')])
        for k in triggered.files:
            if '/daq_' in k or '/pulse_' in k or '/trigger_' in k:          # (the flat hits of a channel come in the order of an atomic)
                assert np.array_equal(bits(triggered[k]), bits(digitised[k])), k
        sim = Simulation(tiny_geometry, seed=4)
        rng = np.random.default_rng(sim.seed)
        events = list(sim.simulate([cli.bomb_event(900, 400.0, [0.0, 0.0, 0.0], rng) for _ in range(2)], keep_hits=False, run_daq=True,
                                   max_steps=100, daq_window=window, daq_trigger=trigger, daq_digitizer=digitizer))
        for k, ev in enumerate(events):
            for name, want in (('trigger_adc', ev.triggers.traces), ('trigger_trace_flags', ev.triggers.trace_flags)):
                got = digitised['ev%d/%s' % (k, name)]
                assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), 'ev%d/%s' % (k, name)
        assert sum(len(ev.triggers.traces) for ev in events) >= 1
        del sim
    finally:
        tools._current = previous
