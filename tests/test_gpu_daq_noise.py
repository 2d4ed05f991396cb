"""The dark noise of the time-binned DAQ on the GPU -- chroma_daq_count_pulses_noise, chroma_daq_acquire_pulses_noise
(k_daq_noise_count / k_daq_noise_emit beside the pulses' own kernels), GPUEventDaq.acquire_pulses(noise=...) and
Simulation.simulate(daq_noise=...) over them -- bit for bit on the comparand of tests/test_daq_noise_host.py: the restated photons
and the restated noise reduced together.  The cases are the ones that module shows to reach the edges; every output array is
longer than what the call may write and pre-filled with a sentinel, which the words beyond must still hold.
"""
import ctypes

import numpy as np
import pytest

from chroma_amd import event
from test_gpu_photon_arrays import (geos, host_geos, gpu, upload, daq_rows, DAQ_BASE, DETECT, SENTINEL, GUARD_WORDS, structure)      # noqa: F401
from test_gpu_daq_events import tables_of, BASE, WEIGHT, ERR_INVALID
from test_gpu_daq_pulses import Outputs, COLUMNS, assert_pulses, acquire_rc, count_rc
from test_daq_pulses_host import W_CUT, SEED
from test_daq_noise_host import noise_cases, expected_with_noise, WINDOWS, LEVELS, NROWS, NOISE, TRIGGER          # noqa: F401

pytestmark = pytest.mark.gpu


class Noise(object):
    """A chroma_daq_noise on the device, and what keeps its arrays alive."""

    def __init__(self, count_cdf, accept, flag=NOISE, ncount=None, null=()):
        from chroma_amd import _lib
        from chroma_amd.gpu.tools import to_gpu
        self.count_cdf = np.ascontiguousarray(count_cdf, dtype=np.uint32)
        self.d_accept = to_gpu(np.ascontiguousarray(accept, dtype=np.uint32))
        self.struct = _lib.DaqNoise(None if 'count_cdf' in null else _lib.ptr(self.count_cdf), len(self.count_cdf) if ncount is None else ncount,
                                    None if 'accept' in null else self.d_accept.ptr, flag)

    @classmethod
    def of(cls, case):
        return cls(case['count_cdf'], case['accept'])


def row_noise_words(nrows):
    from chroma_amd.gpu.tools import to_gpu
    return to_gpu(np.full(nrows + GUARD_WORDS, SENTINEL, dtype=np.uint32))


def call_args(gpu, geo, daq, dev, bounds, window, noise, rng=None, nphotons=None):
    from chroma_amd import _lib
    ctx = gpu.get_context()
    bounds = np.ascontiguousarray(bounds, dtype=np.uint32)
    s = structure(dev)
    win = _lib.DaqWindow(*window)
    keep = (bounds, s, win, noise)
    return keep, (ctx.handle, geo.gg.handle, ctypes.byref(daq.tables), len(bounds) - 1, _lib.ptr(bounds), DETECT, ctypes.byref(s),
                  len(dev.pos) if nphotons is None else nphotons, _lib.Rng(SEED, DAQ_BASE) if rng is None else rng, BASE, WEIGHT,
                  ctypes.byref(win), None if noise is None else ctypes.byref(noise.struct))


def count_noise_rc(gpu, *args, **kw):
    keep, a = call_args(gpu, *args, **kw)
    naccepted = ctypes.c_uint64(SENTINEL)
    rc = gpu.get_context()._lib.chroma_daq_count_pulses_noise(*(a + (ctypes.byref(naccepted),)))
    return rc, int(naccepted.value)


def acquire_noise_rc(gpu, out, row_noise, *args, capacity=None, **kw):
    keep, a = call_args(gpu, *args, **kw)
    npulses = ctypes.c_uint64(SENTINEL)
    rc = gpu.get_context()._lib.chroma_daq_acquire_pulses_noise(*(a + (out.capacity if capacity is None else capacity,) + tuple(out.pointers()) +
                                                                  (None if row_noise is None else row_noise.ptr, ctypes.byref(npulses))))
    return rc, int(npulses.value)


def assert_row_noise(row_noise, want, what):
    got = row_noise.get()
    assert np.array_equal(got[:len(want)], want), what + ': noise per row'
    assert (got[len(want):] == SENTINEL).all(), what + ': guard words behind the noise per row'


# ---- 1. count and acquire are the comparand, case by case -------------------------------------------------------------------------
@pytest.mark.parametrize('nrows', NROWS)
@pytest.mark.parametrize('which', ['tiny', 'stress'])
def test_count_and_acquire_are_the_comparand(gpu, geos, noise_cases, which, nrows):
    from chroma_amd import _lib
    geo = geos[which]
    daq = tables_of(gpu, geo)
    dev = None
    for wname in WINDOWS:
        for level in LEVELS:
            case = noise_cases(which, nrows, wname, level)
            dev = upload(case['rows']) if dev is None else dev
            what = '%s, %d rows, %s, %s' % (which, nrows, wname, level)
            want, noise = case['want'], Noise.of(case)
            rc, naccepted = count_noise_rc(gpu, geo, daq, dev, case['bounds'], case['window'], noise)
            _lib.check(rc)
            assert naccepted == want['naccepted'], what
            out, row_noise = Outputs(nrows, naccepted), row_noise_words(nrows)
            rc, npulses = acquire_noise_rc(gpu, out, row_noise, geo, daq, dev, case['bounds'], case['window'], noise)
            _lib.check(rc)
            assert_pulses(out, npulses, want, what)
            assert_row_noise(row_noise, want['row_noise'], what)


# ---- 2. no photons at all -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('level', list(LEVELS))
def test_a_call_without_photons_has_its_noise(gpu, geos, noise_cases, level):
    """All bounds equal: the photon span is empty, no photon kernel runs, the rows' noise is there all the same; without noise such
    a call writes zeros."""
    from chroma_amd import _lib
    geo = geos['tiny']
    case = noise_cases('tiny', 3, 'cut', level)
    want = expected_with_noise(case['acc'][:0], case['kept'], W_CUT, 3, geo.nchannels)
    assert want['naccepted'] == len(case['kept']) and (level == 'low' or len(want['npe']) > 10)
    daq, dev, noise = tables_of(gpu, geo), upload(case['rows']), Noise.of(case)
    for at in (0, 300, len(case['rows'][0])):
        bounds = [at] * 4
        rc, naccepted = count_noise_rc(gpu, geo, daq, dev, bounds, W_CUT, noise)
        _lib.check(rc)
        assert naccepted == want['naccepted']
        out, row_noise = Outputs(3, naccepted + 1), row_noise_words(3)
        rc, npulses = acquire_noise_rc(gpu, out, row_noise, geo, daq, dev, bounds, W_CUT, noise)
        _lib.check(rc)
        assert_pulses(out, npulses, want, 'no photons, bounds at %d' % at)
        assert_row_noise(row_noise, want['row_noise'], 'no photons')
    out, row_noise = Outputs(3, 4), row_noise_words(3)
    rc, npulses = acquire_noise_rc(gpu, out, row_noise, geo, daq, dev, [300] * 4, W_CUT, None)
    assert rc == 0 and npulses == 0
    assert_row_noise(row_noise, np.zeros(3, dtype=np.uint32), 'no photons, no noise')
    assert (out.get()['offsets'][:4] == 0).all() and (out.get()['outside'][:6] == 0).all()


# ---- 3. NULL is the existing calls; a call is repeatable ------------------------------------------------------------------------------
@pytest.mark.parametrize('which', ['tiny', 'stress'])
def test_null_noise_is_the_existing_calls_and_two_calls_give_the_same_bits(gpu, geos, noise_cases, which):
    from chroma_amd import _lib
    geo = geos[which]
    case = noise_cases(which, 70, 'cut', 'high')
    nrows, bounds, window = 70, case['bounds'], case['window']
    daq, dev = tables_of(gpu, geo), upload(case['rows'])
    rc, plain_count = count_rc(gpu, geo, daq, dev, bounds, window)
    _lib.check(rc)
    rc, naccepted = count_noise_rc(gpu, geo, daq, dev, bounds, window, None)
    _lib.check(rc)
    assert naccepted == plain_count > 0
    plain = Outputs(nrows, plain_count)
    rc, plain_pulses = acquire_rc(gpu, plain, geo, daq, dev, bounds, window)
    _lib.check(rc)
    out, row_noise = Outputs(nrows, plain_count), row_noise_words(nrows)
    rc, npulses = acquire_noise_rc(gpu, out, row_noise, geo, daq, dev, bounds, window, None)
    _lib.check(rc)
    assert npulses == plain_pulses > 0
    a, b = plain.get(), out.get()
    assert all(np.array_equal(a[name], b[name]) for name in a), 'noise = NULL is not chroma_daq_acquire_pulses'
    assert_row_noise(row_noise, np.zeros(nrows, dtype=np.uint32), 'noise = NULL')
    rc, npulses = acquire_noise_rc(gpu, out, None, geo, daq, dev, bounds, window, None)          # (no room for the noise per row: fine)
    _lib.check(rc)
    # the same call twice: the entries' positions come from an atomic, the output does not show it
    noise = Noise.of(case)
    runs = []
    for attempt in range(2):
        out, row_noise = Outputs(nrows, case['want']['naccepted']), row_noise_words(nrows)
        rc, npulses = acquire_noise_rc(gpu, out, row_noise, geo, daq, dev, bounds, window, noise)
        _lib.check(rc)
        runs.append((npulses, out.get(), row_noise.get()))
    assert runs[0][0] == runs[1][0] == len(case['want']['npe']) > plain_pulses
    assert all(np.array_equal(runs[0][1][name], runs[1][1][name]) for name in runs[0][1]) and np.array_equal(runs[0][2], runs[1][2])
    # all-zero accept words: noise that keeps nothing is no noise
    nothing = Noise(case['count_cdf'], np.zeros(geo.nchannels, dtype=np.uint32))
    out, row_noise = Outputs(nrows, plain_count), row_noise_words(nrows)
    rc, npulses = acquire_noise_rc(gpu, out, row_noise, geo, daq, dev, bounds, window, nothing)
    _lib.check(rc)
    b = out.get()
    assert npulses == plain_pulses and all(np.array_equal(a[name], b[name]) for name in a)


# ---- 4. chunks, and the trigger -----------------------------------------------------------------------------------------------------
def assert_event_pulses(pulses, want, nrows, what):
    assert len(pulses) == nrows and np.array_equal(pulses.offsets, want['offsets']), what
    assert np.array_equal(np.array([pulses.outside(r) for r in range(nrows)]).reshape(-1), want['outside']), what
    assert pulses.noise.dtype == np.uint32 and np.array_equal(pulses.noise, want['row_noise']), what + ': noise per event'
    for name in COLUMNS:
        assert np.array_equal(getattr(pulses, name).view(np.uint32), want[name].view(np.uint32)), '%s: %s' % (what, name)


@pytest.mark.parametrize('level', list(LEVELS))
def test_the_chunking_does_not_show_and_the_trigger_sees_the_noise(gpu, geos, noise_cases, level):
    """70 events in chunks of 16, of 1 and in one: the comparand each time.  With a trigger the device triggers what
    EventPulses.trigger computes from the returned pulses, and noise fires it where light alone does not."""
    from chroma_amd import _lib
    geo = geos['tiny']
    case = noise_cases('tiny', 70, 'all', level)
    want, bounds, window = case['want'], case['bounds'], case['window']
    dev = upload(case['rows'])
    rng = _lib.Rng(SEED, DAQ_BASE)
    trigger = gpu.DaqTrigger(*TRIGGER, kind='nhit')
    fired = {}
    for rows_per_chunk in (16, 1, None):
        if rows_per_chunk is None:
            event_daq = gpu.GPUEventDaq(geo.gg)
            assert event_daq.rows_per_chunk >= 70
        else:
            event_daq = gpu.GPUEventDaq(geo.gg, max_entries=rows_per_chunk * geo.nchannels)
            assert event_daq.rows_per_chunk == rows_per_chunk
        what = '%d rows per chunk' % event_daq.rows_per_chunk
        pulses = event_daq.acquire_pulses(dev, rng, bounds, window, acquisition=BASE, weight=WEIGHT, noise=case['noise'], trigger=trigger)
        assert_event_pulses(pulses, want, 70, what)
        one = pulses.event(20)
        assert one.noise == want['row_noise'][20] and pulses.event(0).noise == want['row_noise'][0]
        host = pulses.trigger(trigger)
        for name in ('offsets', 'bin', 'sum', 'hit_offsets', 'hit_channel', 'hit_npe', 'hit_q_int', 'hit_flags', 'pulse_trigger'):
            assert np.array_equal(getattr(pulses.triggers, name), getattr(host, name)), '%s: triggers.%s' % (what, name)
        assert np.array_equal(pulses.triggers.hit_t_first.view(np.uint32), host.hit_t_first.view(np.uint32)), what
        fired[rows_per_chunk] = len(pulses.triggers.bin)
        # noise that is off, and no noise, are the plain pulses
        if rows_per_chunk == 16:
            plain = event_daq.acquire_pulses(dev, rng, bounds, window, acquisition=BASE, weight=WEIGHT, trigger=trigger)
            off = event_daq.acquire_pulses(dev, rng, bounds, window, acquisition=BASE, weight=WEIGHT, noise=0.0)
            assert not plain.noise.any() and not off.noise.any() and len(plain.npe) == len(off.npe) < len(pulses.npe)
            assert all(np.array_equal(getattr(plain, name).view(np.uint32), getattr(off, name).view(np.uint32)) for name in COLUMNS)
            assert not (plain.flags & NOISE).any() and (pulses.flags & NOISE).any()
            fired['plain'] = len(plain.triggers.bin)
    assert fired[16] == fired[1] == fired[None]
    if level == 'high':
        assert fired[None] >= fired['plain'] + 5, 'the noise fires no trigger'          # (tests/test_daq_noise_host.py shows that it does)


# ---- 5. capacity --------------------------------------------------------------------------------------------------------------------
def test_a_capacity_one_short_is_refused_with_the_count_and_nothing_is_written(gpu, geos, noise_cases):
    from chroma_amd import _lib
    geo = geos['tiny']
    case = noise_cases('tiny', 70, 'cut', 'high')
    want = case['want']
    n = len(want['npe'])
    daq, dev, noise = tables_of(gpu, geo), upload(case['rows']), Noise.of(case)
    out, row_noise = Outputs(70, n - 1), row_noise_words(70)
    rc, npulses = acquire_noise_rc(gpu, out, row_noise, geo, daq, dev, case['bounds'], case['window'], noise)
    assert rc == ERR_INVALID and npulses == n
    gpu.get_context().synchronize()
    out.assert_untouched('capacity %d of %d' % (n - 1, n))
    assert (row_noise.get() == SENTINEL).all(), 'the noise per row was written'
    out, row_noise = Outputs(70, n), row_noise_words(70)
    rc, npulses = acquire_noise_rc(gpu, out, row_noise, geo, daq, dev, case['bounds'], case['window'], noise)
    _lib.check(rc)
    assert_pulses(out, npulses, want, 'capacity == npulses')
    assert_row_noise(row_noise, want['row_noise'], 'capacity == npulses')


# ---- 6. refusals before anything is launched ------------------------------------------------------------------------------------------
def test_bad_noise_is_refused_before_anything_is_launched(gpu, geos, noise_cases):
    from chroma_amd import _lib
    geo = geos['tiny']
    case = noise_cases('tiny', 3, 'cut', 'high')
    daq, dev = tables_of(gpu, geo), upload(case['rows'])
    cdf, accept, bounds = case['count_cdf'], case['accept'], case['bounds']
    n = len(dev.pos)
    good = Noise(cdf, accept)
    top = 0xffffffff << 32
    cases = [('no entries', dict(noise=Noise(cdf, accept, ncount=0))),
             ('65 entries', dict(noise=Noise(np.full(65, 2 ** 32 - 1, dtype=np.uint32), accept))),
             ('a descending table', dict(noise=Noise(cdf[::-1], accept))),
             ('no flag', dict(noise=Noise(cdf, accept, flag=0))), ('two flags', dict(noise=Noise(cdf, accept, flag=NOISE | DETECT))),
             ('no table', dict(noise=Noise(cdf, accept, null=('count_cdf',)))), ('no accept words', dict(noise=Noise(cdf, accept, null=('accept',)))),
             ('ids in the high word', dict(noise=good, rng=_lib.Rng(SEED, top))), ('ids in the high word from the first on', dict(noise=good, rng=_lib.Rng(SEED, top + 5))),
             ('ids that reach the high word', dict(noise=good, rng=_lib.Rng(SEED, top - n + 1))),
             ('what the plain calls refuse: dt = 0', dict(noise=good, window=(0.0, 0.0, 8))),
             ('what the plain calls refuse: descending bounds', dict(noise=good, bounds=[300, 299, 400, 500])),
             ('what the plain calls refuse: beyond the set', dict(noise=good, bounds=[300, 400, 500, n + 1]))]
    assert len(cdf) >= 3 and cdf[0] < cdf[-1]
    out, row_noise = Outputs(3, 4000), row_noise_words(3)
    for what, kw in cases:
        kw = dict(dict(bounds=bounds, window=W_CUT), **kw)
        args = (geo, daq, dev, kw.pop('bounds'), kw.pop('window'), kw.pop('noise'))
        rc, naccepted = count_noise_rc(gpu, *args, **kw)
        assert rc == ERR_INVALID and naccepted == SENTINEL, what + ' (count)'
        rc, npulses = acquire_noise_rc(gpu, out, row_noise, *args, **kw)
        assert rc == ERR_INVALID and npulses == SENTINEL, what
    gpu.get_context().synchronize()
    out.assert_untouched('refused calls')
    assert (row_noise.get() == SENTINEL).all()
    # the last id below the high word is fine, and without noise the ids are not looked at
    rc, naccepted = count_noise_rc(gpu, geo, daq, dev, bounds, W_CUT, good, rng=_lib.Rng(SEED, top - n))
    assert rc == 0 and naccepted >= len(case['kept'])
    rc, naccepted = count_noise_rc(gpu, geo, daq, dev, bounds, W_CUT, None, rng=_lib.Rng(SEED, top))
    assert rc == 0


# ---- 7. through Simulation ------------------------------------------------------------------------------------------------------------
def bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def test_simulation_draws_the_noise_into_the_pulses_and_not_into_the_channels(gpu, tiny_geometry, tmp_path):
    """A few bomb events and an empty one through Simulation.simulate(run_daq=True, daq_window=...) with and without daq_noise, same
    seed: ev.channels is the same bit for bit; ev.pulses is what GPUEventDaq.acquire_pulses gives for the events' final photons
    under the simulation's seed and first photon id; the empty event has noise alone; chroma-sim --daq-noise writes the pulses' flags
    and the noise count of every event."""
    from conftest import bomb
    from chroma_amd import _lib
    from chroma_amd.gpu import tools
    from chroma_amd.sim import Simulation
    previous = tools._current
    window = (-8.0, 0.5, 512)
    rate = 2.0e6          # (0.5 candidates per channel and event)
    trigger = (6, 4)
    try:
        runs = {}
        for with_noise in (False, True):
            batch = [bomb(n, seed=300 + k) for k, n in enumerate([400, 1, 3000, 64])]
            batch.insert(2, event.Photons())
            sim = Simulation(tiny_geometry, seed=21)
            with pytest.raises(ValueError):
                list(sim.simulate(iter(()), run_daq=True, daq_noise=rate))          # (no window: before anything is looked at)
            with pytest.raises(ValueError):
                list(sim.simulate(batch, run_daq=True, daq_window=window, daq_noise=-1.0))
            with pytest.raises(ValueError):
                list(sim.simulate(batch, run_daq=True, daq_window=window, daq_noise=1e9))          # (256 candidates per word)
            kw = dict(daq_noise=rate) if with_noise else {}
            runs[with_noise] = list(sim.simulate(batch, run_daq=True, max_steps=100, keep_photons_end=True, daq_window=window, daq_trigger=trigger, **kw))
            if with_noise:
                ends = [ev.photons_end for ev in runs[True]]
                bounds = np.cumsum([0] + [len(p) for p in ends])
                dev = gpu.GPUPhotons(event.Photons.join(ends))
                direct = gpu.GPUEventDaq(sim.gpu_geometry).acquire_pulses(dev, _lib.Rng(sim.rng_states.seed, 0), bounds, window, acquisition=0,
                                                                          noise=gpu.DaqNoise(rate), trigger=trigger)
            del sim
        nnoise = 0
        for i, (plain, ev) in enumerate(zip(runs[False], runs[True])):
            for name in ('t', 'q', 'flags', 'hit'):
                assert np.array_equal(bits(getattr(ev.channels, name)), bits(getattr(plain.channels, name))), 'event %d: channels.%s' % (i, name)
            assert plain.pulses.noise == 0 and not (plain.pulses.flags & event.DARK_NOISE).any()
            p, want = ev.pulses, direct.event(i)
            for name in ('channel', 'bin', 'npe', 'q_int', 't_first', 'flags', 'q'):
                assert np.array_equal(bits(getattr(p, name)), bits(getattr(want, name))), 'event %d: pulses.%s' % (i, name)
            assert (p.early, p.late, p.noise) == (want.early, want.late, want.noise) and (p.early, p.late) == (plain.pulses.early, plain.pulses.late)
            assert p.npe.sum() == plain.pulses.npe.sum() + p.noise and p.npe[(p.flags & event.DARK_NOISE) != 0].sum() >= p.noise
            assert np.array_equal(ev.triggers.bin, direct.triggers.event(i).bin)
            nnoise += p.noise
        empty = runs[True][2].pulses
        assert len(runs[False][2].pulses) == 0 and len(empty) > 0 and (empty.flags == event.DARK_NOISE).all() and empty.npe.sum() == empty.noise
        assert nnoise > 20
        # chroma-sim --daq-noise: the pulses' flags and the event's noise count beside the arrays of --daq-window
        from chroma_amd import cli
        files = {}
        for name, extra in (('plain', []), ('noise', ['--daq-noise', '2e6'])):
            files[name] = str(tmp_path / (name + '.npz'))
            argv = ['@chroma_amd.demo.tiny', '-n', '2', '--nphotons', '900', '-s', '4', '--max-steps', '100', '-o', files[name], '--daq-window=-8,0.5,512']
            assert cli.main(argv + extra) == 0
        plain, noisy = np.load(files['plain']), np.load(files['noise'])
        assert sorted(noisy.files) == sorted(plain.files + ['ev%d/pulse_%s' % (k, name) for k in range(2) for name in ('flags', 'noise')])
        for k in range(2):
            flags, count = noisy['ev%d/pulse_flags' % k], int(noisy['ev%d/pulse_noise' % k])
            assert len(flags) == len(noisy['ev%d/pulse_npe' % k]) and count > 0
            assert noisy['ev%d/pulse_npe' % k].sum() == plain['ev%d/pulse_npe' % k].sum() + count
            assert noisy['ev%d/pulse_npe' % k][(flags & event.DARK_NOISE) != 0].sum() >= count
            for name in ('daq_hit', 'daq_t', 'daq_q'):
                key = 'ev%d/%s' % (k, name)
                assert key in plain.files and np.array_equal(bits(plain[key]), bits(noisy[key])), key
    finally:
        tools._current = previous
