"""The trace reduction of the time-binned DAQ on the GPU -- chroma_daq_reduce_traces (k_daq_reduce_count, k_daq_reduce_fill),
GPUEventDaq.acquire_pulses(reducer=...) and Simulation.simulate(daq_reducer=...) over it -- bit for bit on the brute-force
restatement of tests/test_daq_reduce_host.py, on that module's traces and reducers (uploaded as they are: the reduction is a
function of the traces) and on what the library itself digitises.  Every output array is longer than what the call may write and
pre-filled with a sentinel, which the words beyond must still hold.
"""
import ctypes

import numpy as np
import pytest

from chroma_amd import event
from test_gpu_photon_arrays import geos, host_geos, gpu, upload, DAQ_BASE      # noqa: F401
from test_gpu_daq_events import BASE, WEIGHT
from test_daq_pulses_host import restated, W_ALL, SEED as PHOTON_SEED          # noqa: F401
from test_daq_reduce_host import (Reducer, brute_reduce, digitised_sets, handmade, full_scale, random_traces, prepare, ORDER, PER_TRACE, PER_PULSE,
                                  assert_reduced, untouched, refusals, refusal_case, ERR_INVALID, SENTINEL_N)

pytestmark = pytest.mark.gpu


def device_reduce(gpu, adc, r, capacity, guard=8, change=None):
    """chroma_daq_reduce_traces into sentinel-filled device arrays `guard` entries longer than the call may write; (rc, the dict of
    prepare() with the arrays read back)."""
    from chroma_amd.gpu.tools import to_gpu
    ctx = gpu.get_context()
    v = prepare(adc, r, capacity, guard, change)
    device = {}
    args = [ctx.handle]
    for k in ORDER:
        a = v[k]
        if isinstance(a, np.ndarray):
            device[k] = to_gpu(a) if len(a) else None
            a = device[k].ptr if len(a) else None
        elif isinstance(a, (ctypes.Structure, ctypes.c_uint64)):
            a = ctypes.byref(a)
        args.append(a)
    rc = ctx._lib.chroma_daq_reduce_traces(*args)
    ctx.synchronize()
    for k, a in device.items():
        if a is not None and k != 'adc':
            v[k] = a.get()
    return rc, v


def run(gpu, adc, r, want, what, **kw):
    from chroma_amd import _lib
    rc, v = device_reduce(gpu, adc, r, len(want['found_start']), **kw)
    _lib.check(rc)
    assert_reduced(v, want, what)


# ---- 1. the call is the restatement ------------------------------------------------------------------------------------------------------
def test_the_call_is_the_restatement_on_the_digitised_trigger_sets(gpu):
    """One call per reducer: the sets of one trace length under one reducer, stacked -- the traces of a call are independent."""
    stacks = {}
    for what, adc, r, want in digitised_sets():
        stacks.setdefault((r.name, adc.shape[1]), []).append((adc, r))
    assert len(stacks) > 40
    for (name, G), members in stacks.items():
        adc = np.concatenate([a for a, _ in members])
        r = members[0][1]
        run(gpu, adc, r, brute_reduce(adc, r), '%s, %d samples' % (name, G))


def test_the_call_is_the_restatement_on_the_handmade_traces(gpu):
    for what, adc, r in handmade() + full_scale():
        run(gpu, adc, r, brute_reduce(adc, r), what)


@pytest.mark.parametrize('ntraces', (1, 3, 4, 5, 300))
def test_the_call_is_the_restatement_at_the_edges_of_a_block_of_four_traces(gpu, ntraces):
    adc, r = random_traces()
    start = int(np.flatnonzero(np.diff(brute_reduce(adc, r)['found_offsets']) >= 2)[0])          # (the first trace is one with pulses)
    pick = adc[start:start + ntraces] if ntraces < 300 else adc
    want = brute_reduce(pick, r)
    assert len(pick) == ntraces and len(want['found_start']) >= 2
    run(gpu, pick, r, want, '%d traces' % ntraces)
    falling = Reducer('falling, baseline of 64', 6, polarity=-1, nbaseline=64, baseline_spread=8, lead=3, lag=3, cfd=77)
    upside_down = (400 - pick.astype(np.int64)).clip(0, 65535).astype(np.uint16)
    run(gpu, upside_down, falling, brute_reduce(upside_down, falling), '%d traces upside down' % ntraces)


# ---- 2. slices and capacities ---------------------------------------------------------------------------------------------------------------
def test_a_slice_of_the_traces_is_that_part_of_the_whole(gpu):
    adc, r = random_traces()
    want = brute_reduce(adc, r)
    for first, n in ((0, 5), (37, 101), (299, 1), (3, 297)):
        f0, f1 = int(want['found_offsets'][first]), int(want['found_offsets'][first + n])
        part = {name: want[name][first:first + n] for name, _ in PER_TRACE[1:]}
        part['found_offsets'] = want['found_offsets'][first:first + n + 1] - np.uint32(f0)
        part.update({name: want[name][f0:f1] for name, _ in PER_PULSE})
        run(gpu, adc[first:first + n], r, part, 'traces [%d, %d)' % (first, first + n))


def test_too_little_room_writes_the_count_and_the_per_trace_arrays_and_leaves_the_pulse_arrays(gpu):
    adc, r = random_traces()
    want = brute_reduce(adc, r)
    nfound = len(want['found_start'])
    for capacity in (0, nfound - 1):
        rc, v = device_reduce(gpu, adc, r, capacity)
        assert rc == ERR_INVALID, capacity
        assert_reduced(v, want, 'room for %d of %d' % (capacity, nfound), filled=False)
    rc, v = device_reduce(gpu, adc, r, nfound)
    assert rc == 0
    assert_reduced(v, want, 'room for all')


def test_what_the_header_refuses_is_refused_before_anything_is_launched_and_no_traces_is_ok(gpu):
    adc, r, nfound = refusal_case()
    names = [name for name, _ in PER_TRACE + PER_PULSE]
    for what, change in refusals():
        rc, v = device_reduce(gpu, adc, r, nfound, change=change)
        assert rc == ERR_INVALID, what
        assert untouched(v, names) and (v['nfound'] is None or v['nfound'].value == SENTINEL_N), what
    for change in ({}, {name: None for name in ['adc'] + names}):
        rc, v = device_reduce(gpu, adc[:0], r, 4, change=change)
        assert rc == 0 and v['nfound'].value == 0 and untouched(v, names)
    rc, v = device_reduce(gpu, adc, r, nfound)
    assert rc == 0
    assert_reduced(v, brute_reduce(adc, r), 'the valid call')


# ---- 3. GPUEventDaq.acquire_pulses(reducer=...) ---------------------------------------------------------------------------------------------------
FOUND = [name for name, _ in PER_TRACE + PER_PULSE]


def test_acquire_pulses_with_a_reducer_is_the_host_twin_whatever_the_chunking_with_and_without_the_traces(gpu, geos, restated):
    from chroma_amd import _lib
    geo = geos['tiny']
    rows, bounds, acc = restated('tiny', 'many')
    dev = upload(rows)
    trigger = gpu.DaqTrigger(1, 4, 8, 2, 6)
    digitizer = gpu.DaqDigitizer.biexponential(40.0, 0.5, 2.0, W_ALL[1], bits=12, pedestal=200, noise_sigma=1.5)
    reducer = gpu.DaqReducer.for_digitizer(digitizer, 6, min_width=1, lead=1, lag=2, cfd=0.4)
    noise = gpu.DaqNoise(2e6)
    results = {}
    for rows_per_chunk in (7, None):
        event_daq = gpu.GPUEventDaq(geo.gg) if rows_per_chunk is None else gpu.GPUEventDaq(geo.gg, max_entries=7 * geo.nchannels + geo.nchannels - 1)
        rng = _lib.Rng(PHOTON_SEED, DAQ_BASE)
        if rows_per_chunk:
            event_daq.max_entries = 40          # (the samples of one digitiser call: slices of 5 traces, each reduced on its own)
        kw = dict(acquisition=BASE, weight=WEIGHT, trigger=trigger, noise=noise, digitizer=digitizer)
        plain = event_daq.acquire_pulses(dev, rng, bounds, W_ALL, **kw).triggers
        t = event_daq.acquire_pulses(dev, rng, bounds, W_ALL, reducer=reducer, **kw).triggers
        dropped = event_daq.acquire_pulses(dev, rng, bounds, W_ALL, reducer=reducer, keep_traces=False, **kw).triggers
        assert plain.reducer is None and plain.found_start is None and t.reducer == reducer and dropped.reducer == reducer
        assert np.array_equal(t.adc, plain.adc) and np.array_equal(t.trace_flags, plain.trace_flags)
        assert dropped.adc is None and np.array_equal(dropped.trace_flags, plain.trace_flags)
        offline = t.reduce(reducer)
        want = brute_reduce(t.adc, Reducer('the same', 6, pedestal=200, lead=1, lag=2, cfd=reducer.cfd))
        for name in FOUND:
            for got, what in ((t, 'with the traces'), (dropped, 'without the traces'), (want, 'the restatement')):
                a = got[name] if isinstance(got, dict) else getattr(got, name)
                assert np.array_equal(a, getattr(offline, name)), '%s, %s, %s rows per chunk' % (name, what, rows_per_chunk)
        assert t.found_offsets.dtype == np.int64 and len(t.found_offsets) == len(t.hit_channel) + 1 and t.found_integral.dtype == np.int64
        results[rows_per_chunk] = t
    for name in FOUND:
        assert np.array_equal(getattr(results[7], name), getattr(results[None], name)), name
    t = results[7]
    per_trace = np.diff(t.found_offsets)
    assert len(t.found_start) > 100 and (per_trace == 0).any() and (per_trace >= 1).sum() > 50
    with pytest.raises(ValueError, match='reducer needs digitizer'):
        event_daq.acquire_pulses(dev, rng, bounds, W_ALL, trigger=trigger, reducer=reducer)
    with pytest.raises(ValueError, match='baseline'):
        event_daq.acquire_pulses(dev, rng, bounds, W_ALL, trigger=trigger, digitizer=digitizer, reducer=gpu.DaqReducer(6, nbaseline=9))


# ---- 4. through Simulation and chroma-sim ------------------------------------------------------------------------------------------------------------
def test_simulation_gives_every_event_what_was_found_in_its_traces_and_chroma_sim_writes_it(gpu, tiny_geometry, tmp_path):
    from conftest import bomb
    from chroma_amd import cli
    from chroma_amd.gpu import tools
    from chroma_amd.sim import Simulation
    previous = tools._current
    window = (-8.0, 0.5, 512)
    trigger = gpu.DaqTrigger(2, 16, 64, 8, 40)
    digitizer = gpu.DaqDigitizer.biexponential(30.0, 1.0, 6.0, 0.5, bits=12, pedestal=150, noise_sigma=2.0)
    reducer = gpu.DaqReducer.for_digitizer(digitizer, 8, lead=2, lag=6, nbaseline=4, min_width=2, time_offset_ns=0.75)
    try:
        runs = {}
        for keep in (True, False):
            batch = [bomb(n, seed=300 + k) for k, n in enumerate([400, 1, 3000, 64])]
            batch.insert(2, event.Photons())
            sim = Simulation(tiny_geometry, seed=21)
            runs[keep] = list(sim.simulate(batch, run_daq=True, max_steps=100, daq_window=window, daq_trigger=trigger, daq_digitizer=digitizer,
                                           daq_reducer=reducer, daq_keep_traces=keep))
            del sim
        npulses = 0
        for ev, dropped in zip(runs[True], runs[False]):
            t, d = ev.triggers, dropped.triggers
            assert isinstance(t, gpu.Triggers) and t.reducer == reducer and d.traces is None and np.array_equal(d.trace_flags, t.trace_flags)
            want = gpu.daq.reduce_traces_host(t.traces, reducer) if len(t.traces) else None
            for k, name in enumerate(FOUND):
                assert np.array_equal(getattr(t, name), getattr(d, name)), 'event %d: %s without the traces' % (ev.id, name)
                if want is not None:
                    assert np.array_equal(getattr(t, name), want[k]), 'event %d: %s' % (ev.id, name)
            for k in range(len(t)):
                channel, tt, q, n, flags = t.reco(k)
                dense = t.reco_channels(k)
                assert isinstance(dense, event.Channels) and np.array_equal(np.flatnonzero(dense.hit), channel)
                assert np.array_equal(dense.t[channel], tt.astype(np.float32)) and np.array_equal(dense.q[channel], q.astype(np.float32))
                if len(channel):
                    f = t.found(k, channel[0])
                    assert len(f) == n[0] and f.t[0] == tt[0]
                    first = int(t.bin[k]) - trigger.pre
                    assert f.t[0] == window[0] + window[1] * (first + float(f.time[0]) / 256.0) - 0.75
                    assert q[0] == pytest.approx(float(f.integral.sum()) / (4 * digitizer.shape.sum()))
                    # what was found is what was there: within the gate's span in time, and a charge of the order of the truth's
                    assert window[0] + window[1] * first - 0.75 <= tt[0] <= window[0] + window[1] * (first + 48)
                npulses += int(n.sum())
        assert npulses >= 3
        # chroma-sim --daq-reduce: the found arrays beside those of --daq-digitize; --daq-drop-traces: without trigger_adc
        files = {}
        base = ['@chroma_amd.demo.tiny', '-n', '2', '--nphotons', '900', '-s', '4', '--max-steps', '100', '--daq-window=-8,0.5,512', '--daq-trigger',
                '2,16,64,8,40', '--daq-digitize', '30,1,6,12,150,2']
        for flag, more in (('digitize', []), ('reduce', ['--daq-reduce', '8,2,6,0.5,4,2']), ('drop', ['--daq-reduce', '8,2,6,0.5,4,2', '--daq-drop-traces'])):
            files[flag] = str(tmp_path / (flag + '.npz'))
            assert cli.main(base + more + ['-o', files[flag]]) == 0
        digitised, reduced, dropped = [np.load(files[k]) for k in ('digitize', 'reduce', 'drop')]
        added = ['trigger_' + name for name in FOUND]
        assert sorted(reduced.files) == sorted(digitised.files + ['ev%d/%s' % (k, name) for k in range(2) for name in added])
        assert sorted(dropped.files) == sorted(k for k in reduced.files if not k.endswith('/trigger_adc'))
        found = 0
        for k in range(2):
            adc = reduced['ev%d/trigger_adc' % k]
            assert np.array_equal(adc, digitised['ev%d/trigger_adc' % k])
            want = gpu.daq.reduce_traces_host(adc, gpu.DaqReducer.for_digitizer(digitizer, 8, lead=2, lag=6, nbaseline=4, min_width=2)) if len(adc) else None
            for j, name in enumerate(FOUND):
                key = 'ev%d/trigger_%s' % (k, name)
                assert np.array_equal(reduced[key], dropped[key]), key
                if want is not None:
                    assert np.array_equal(reduced[key], want[j]), key
            found += len(reduced['ev%d/trigger_found_start' % k])
        assert found >= 1
    finally:
        tools._current = previous
