"""The time-binned DAQ on the GPU -- chroma_daq_count_pulses, chroma_daq_acquire_pulses (k_daq_pulses_count / _emit, a radix
sort, _heads, a scan, _open, _reduce, _finish), GPUEventDaq.acquire_pulses / EventPulses and Simulation.simulate(daq_window=...)
over them -- bit for bit on the NumPy restatement of tests/test_daq_pulses_host.py, which that module shows to be the oracle's
DAQ.  The photons, events and windows are the ones that module shows to reach the edges; every output array is longer than
what the call may write and pre-filled with a sentinel, which the words beyond must still hold.
"""
import ctypes

import numpy as np
import pytest

from chroma_amd import event
from test_gpu_photon_arrays import (geos, host_geos, gpu, upload, daq_rows, DAQ_BASE, DETECT, SENTINEL, GUARD_WORDS, structure)      # noqa: F401
from test_gpu_daq_events import (tables_of, device_state, acquire_events, call, BASE, WEIGHT, RESET_BITS, ERR_INVALID)
from test_daq_pulses_host import restated, expected_pulses, edge_windows, W_ALL, W_CUT, W_FINE, W_ONE, SEED          # noqa: F401

pytestmark = pytest.mark.gpu

COLUMNS = ('channel', 'bin', 'npe', 'q_int', 't_first', 'flags')


class Outputs(object):
    """The device outputs of one chroma_daq_acquire_pulses call, sentinel-filled: offsets (nrows + 1), the six pulse arrays
    (capacity), outside (2 nrows), GUARD_WORDS more each."""

    def __init__(self, nrows, capacity):
        from chroma_amd.gpu.tools import to_gpu
        fill = lambda n: to_gpu(np.full(n + GUARD_WORDS, SENTINEL, dtype=np.uint32))
        self.nrows, self.capacity = nrows, capacity
        self.offsets, self.outside = fill(nrows + 1), fill(2 * nrows)
        self.columns = [fill(capacity) for _ in COLUMNS]

    def pointers(self, null_columns=False):
        return [self.offsets.ptr] + [None if null_columns else a.ptr for a in self.columns] + [self.outside.ptr]

    def get(self):
        return dict(zip(('offsets', 'outside') + COLUMNS, [a.get() for a in [self.offsets, self.outside] + self.columns]))

    def assert_untouched(self, what):
        for name, a in self.get().items():
            assert (a == SENTINEL).all(), '%s: %s was written' % (what, name)


def pulse_args(gpu, geo, daq, dev, bounds, window, nrows=None, acquisition=BASE, nphotons=None):
    from chroma_amd import _lib
    ctx = gpu.get_context()
    bounds = np.ascontiguousarray(bounds, dtype=np.uint32)
    s = structure(dev)
    win = _lib.DaqWindow(*window)
    keep = (bounds, s, win)
    return keep, (ctx.handle, geo.gg.handle, ctypes.byref(daq.tables), len(bounds) - 1 if nrows is None else nrows, _lib.ptr(bounds), DETECT,
                  ctypes.byref(s), len(dev.pos) if nphotons is None else nphotons, _lib.Rng(SEED, DAQ_BASE), acquisition, WEIGHT, ctypes.byref(win))


def count_rc(gpu, *args, **kw):
    keep, a = pulse_args(gpu, *args, **kw)
    naccepted = ctypes.c_uint64(SENTINEL)
    rc = gpu.get_context()._lib.chroma_daq_count_pulses(*(a + (ctypes.byref(naccepted),)))
    return rc, int(naccepted.value)


def acquire_rc(gpu, out, *args, null_columns=False, capacity=None, **kw):
    keep, a = pulse_args(gpu, *args, **kw)
    npulses = ctypes.c_uint64(SENTINEL)
    rc = gpu.get_context()._lib.chroma_daq_acquire_pulses(*(a + (out.capacity if capacity is None else capacity,) + tuple(out.pointers(null_columns)) +
                                                            (ctypes.byref(npulses),)))
    return rc, int(npulses.value)


def assert_pulses(out, npulses, want, what):
    got = out.get()
    n = len(want['npe'])
    assert npulses == n == want['offsets'][-1], '%s: %d pulses, expected %d' % (what, npulses, n)
    assert np.array_equal(got['offsets'][:out.nrows + 1], want['offsets']), what + ': offsets'
    assert np.array_equal(got['outside'][:2 * out.nrows], want['outside']), what + ': outside'
    for name in COLUMNS:
        assert np.array_equal(got[name][:n], want[name].view(np.uint32)), '%s: %s' % (what, name)
        assert (got[name][n:] == SENTINEL).all() and len(got[name]) == out.capacity + GUARD_WORDS, '%s: words behind the pulses of %s' % (what, name)
    assert (got['offsets'][out.nrows + 1:] == SENTINEL).all(), what + ': guard words behind the offsets'
    assert (got['outside'][2 * out.nrows:] == SENTINEL).all(), what + ': guard words behind the outside counts'


def windows_of(acc):
    on_a, to_b, a, b = edge_windows(acc)
    return [('all', W_ALL), ('cut', W_CUT), ('t0 on a photon', on_a), ('one bin to a photon', to_b), ('fine', W_FINE)]


# ---- 1. count and acquire are the restatement, window by window -----------------------------------------------------------------
@pytest.mark.parametrize('which', ['tiny', 'stress'])
def test_count_and_acquire_are_the_restatement(gpu, geos, restated, which):
    from chroma_amd import _lib
    geo = geos[which]
    rows, bounds, acc = restated(which)
    nrows = len(bounds) - 1
    daq = tables_of(gpu, geo)
    dev = upload(rows)
    for what, window in windows_of(acc):
        what = '%s, %s' % (which, what)
        want = expected_pulses(acc, window, nrows, geo.nchannels)
        rc, naccepted = count_rc(gpu, geo, daq, dev, bounds, window)
        _lib.check(rc)
        assert naccepted == want['naccepted'], what
        assert len(want['npe']) <= naccepted
        out = Outputs(nrows, naccepted)
        rc, npulses = acquire_rc(gpu, out, geo, daq, dev, bounds, window)
        _lib.check(rc)
        assert_pulses(out, npulses, want, what)


# ---- 2. the same photoelectrons as the existing DAQ -----------------------------------------------------------------------------
@pytest.mark.parametrize('which', ['tiny', 'stress'])
def test_the_pulses_sum_to_the_channels_of_acquire_events(gpu, geos, restated, which):
    """The same call arguments through chroma_daq_acquire_events: with the window that holds everything, per (row, channel) the
    sum of q_int is the charge word, the OR of flags the history word and the unsigned minimum of the t_first bits against the
    reset value's the time word."""
    from chroma_amd import _lib
    geo = geos[which]
    rows, bounds, acc = restated(which)
    nrows, nch = len(bounds) - 1, geo.nchannels
    words = nrows * nch
    daq = tables_of(gpu, geo)
    dev = upload(rows)
    arrays = device_state(gpu, words)
    call(gpu, 'chroma_daq_reset', 1e9, words, arrays[0].ptr, arrays[1].ptr, arrays[2].ptr)
    acquire_events(gpu, geo, daq, dev, bounds, arrays)
    t_word, q_word, h_word = [a.get()[:words] for a in arrays]
    out = Outputs(nrows, len(acc))
    rc, npulses = acquire_rc(gpu, out, geo, daq, dev, bounds, W_ALL)
    _lib.check(rc)
    got = out.get()
    row = np.repeat(np.arange(nrows), np.diff(got['offsets'][:nrows + 1].astype(np.int64)))
    word = row * nch + got['channel'][:npulses].view(np.int32)
    q = np.zeros(words, dtype=np.uint64)
    np.add.at(q, word, got['q_int'][:npulses].astype(np.uint64))
    h = np.zeros(words, dtype=np.uint32)
    np.bitwise_or.at(h, word, got['flags'][:npulses])
    t = np.full(words, RESET_BITS, dtype=np.uint32)
    np.minimum.at(t, word, got['t_first'][:npulses])
    assert npulses > 100 and (h_word != 0).sum() >= 10
    assert np.array_equal(q.astype(np.uint32), q_word) and np.array_equal(h, h_word) and np.array_equal(t, t_word)


# ---- 3. many events, and the chunking -------------------------------------------------------------------------------------------
def test_many_events_and_the_result_does_not_depend_on_the_chunking(gpu, geos, restated):
    """Some 1300 events of zero to three photons, more than 2^16 (row, channel) words: the call is the restatement, and
    GPUEventDaq.acquire_pulses with 1, 7 and the default rows per chunk gives the same EventPulses, the restatement's."""
    from chroma_amd import _lib
    geo = geos['tiny']
    rows, bounds, acc = restated('tiny', 'many')
    nrows = len(bounds) - 1
    want = expected_pulses(acc, W_ALL, nrows, geo.nchannels)
    daq = tables_of(gpu, geo)
    dev = upload(rows)
    out = Outputs(nrows, want['naccepted'])
    rc, npulses = acquire_rc(gpu, out, geo, daq, dev, bounds, W_ALL)
    _lib.check(rc)
    assert_pulses(out, npulses, want, 'many rows')
    cut = expected_pulses(acc, W_CUT, nrows, geo.nchannels)
    for rows_per_chunk in (1, 7, None):
        if rows_per_chunk is None:
            event_daq = gpu.GPUEventDaq(geo.gg)
            assert event_daq.rows_per_chunk >= nrows
        else:
            event_daq = gpu.GPUEventDaq(geo.gg, max_entries=rows_per_chunk * geo.nchannels + (geo.nchannels - 1 if rows_per_chunk > 1 else 0))
            assert event_daq.rows_per_chunk == rows_per_chunk
        what = '%d rows per chunk' % event_daq.rows_per_chunk
        for window, expect in ((W_ALL, want), (W_CUT, cut)):
            pulses = event_daq.acquire_pulses(dev, _lib.Rng(SEED, DAQ_BASE), bounds, window, acquisition=BASE, weight=WEIGHT)
            assert isinstance(pulses, gpu.EventPulses) and len(pulses) == nrows, what
            assert np.array_equal(pulses.offsets, expect['offsets']), what
            assert np.array_equal([pulses.outside(r) for r in range(nrows)], expect['outside'].reshape(nrows, 2)), what
            for name in COLUMNS:
                assert np.array_equal(getattr(pulses, name).view(np.uint32), expect[name].view(np.uint32)), '%s: %s' % (what, name)
            unit = np.float32(event_daq.charge_unit)
            assert np.array_equal(pulses.q.view(np.uint32), (expect['q_int'].astype(np.float32) * unit).astype(np.float32).view(np.uint32)), what
        r = int(np.argmax(np.diff(cut['offsets'].astype(np.int64))))
        w = slice(cut['offsets'][r], cut['offsets'][r + 1])
        got = pulses.sparse(r)
        assert np.array_equal(got[0], cut['channel'][w]) and np.array_equal(got[1], cut['bin'][w]) and np.array_equal(got[2], cut['npe'][w])
        assert pulses.outside(r) == tuple(cut['outside'].reshape(-1, 2)[r])
        npe, q = pulses.waveform(r, int(cut['channel'][w][0]))
        assert npe.sum() == cut['npe'][w][cut['channel'][w] == cut['channel'][w][0]].sum() and len(npe) == W_CUT[2]


# ---- 4. one key over many waves -------------------------------------------------------------------------------------------------
def test_one_pulse_of_a_long_run_twice_on_one_context(gpu, geos, restated):
    """'stress', every photon as one event, one bin: the single pulse is the restatement's; a second run on the same context
    (the pooled scratch is there already) gives the same bits."""
    from chroma_amd import _lib
    geo = geos['stress']
    rows, bounds, acc = restated('stress', 'whole')
    want = expected_pulses(acc, W_ONE, 1, 1)
    assert want['npe'][0] > 512
    daq = tables_of(gpu, geo)
    dev = upload(rows)
    for attempt in ('first', 'second'):
        out = Outputs(1, want['naccepted'])
        rc, npulses = acquire_rc(gpu, out, geo, daq, dev, bounds, W_ONE)
        _lib.check(rc)
        assert_pulses(out, npulses, want, 'the long run, %s call' % attempt)


@pytest.mark.parametrize('which', ['tiny', 'stress'])
def test_one_event_with_early_and_late_photons(gpu, geos, restated, which):
    """Every photon of the set as one event under the window that cuts: every block of the emit lies in one row, and adds its
    early and late photons once per block."""
    from chroma_amd import _lib
    geo = geos[which]
    rows, bounds, acc = restated(which, 'whole')
    want = expected_pulses(acc, W_CUT, 1, geo.nchannels)
    assert want['outside'][0] > 64 and want['outside'][1] > 64 and len(rows[0]) > 3 * 1024
    out = Outputs(1, want['naccepted'])
    rc, npulses = acquire_rc(gpu, out, geo, tables_of(gpu, geo), upload(rows), bounds, W_CUT)
    _lib.check(rc)
    assert_pulses(out, npulses, want, which + ', one event')


# ---- 5. capacity ----------------------------------------------------------------------------------------------------------------
def test_a_capacity_one_short_is_refused_with_the_count(gpu, geos, restated):
    from chroma_amd import _lib
    geo = geos['tiny']
    rows, bounds, acc = restated('tiny')
    nrows = len(bounds) - 1
    want = expected_pulses(acc, W_CUT, nrows, geo.nchannels)
    n = len(want['npe'])
    daq = tables_of(gpu, geo)
    dev = upload(rows)
    out = Outputs(nrows, n - 1)
    rc, npulses = acquire_rc(gpu, out, geo, daq, dev, bounds, W_CUT)
    assert rc == ERR_INVALID and npulses == n
    gpu.get_context().synchronize()
    out.assert_untouched('capacity %d of %d' % (n - 1, n))
    out = Outputs(nrows, n)
    rc, npulses = acquire_rc(gpu, out, geo, daq, dev, bounds, W_CUT)
    _lib.check(rc)
    assert_pulses(out, npulses, want, 'capacity == npulses')


# ---- 6. refusals before anything is launched --------------------------------------------------------------------------------------
def test_bad_windows_bounds_and_outputs_are_refused_before_anything_is_launched(gpu, geos):
    from chroma_amd import _lib
    geo = geos['tiny']
    rows = daq_rows(geo)
    n = len(rows[0])
    dev = upload(rows)
    daq = tables_of(gpu, geo)
    good = [257, 300, 400, 500, 600]
    nrows = len(good) - 1
    out = Outputs(nrows, 400)
    cases = [('dt = 0', dict(bounds=good, window=(0.0, 0.0, 8))), ('dt < 0', dict(bounds=good, window=(0.0, -0.5, 8))),
             ('dt NaN', dict(bounds=good, window=(0.0, float('nan'), 8))), ('dt infinite', dict(bounds=good, window=(0.0, float('inf'), 8))),
             ('no bins', dict(bounds=good, window=(0.0, 0.5, 0))), ('65537 bins', dict(bounds=good, window=(0.0, 0.5, 65537))),
             ('descending', dict(bounds=[257, 300, 299, 400, 500], window=W_CUT)),
             ('beyond the set', dict(bounds=[257, 300, 400, 500, n + 1], window=W_CUT)),
             ('no rows', dict(bounds=[257], nrows=0, window=W_CUT))]
    for what, kw in cases:
        rc, naccepted = count_rc(gpu, geo, daq, dev, **kw)
        assert rc == ERR_INVALID and naccepted == SENTINEL, what + ' (count)'
        rc, npulses = acquire_rc(gpu, out, geo, daq, dev, **kw)
        assert rc == ERR_INVALID and npulses == SENTINEL, what
    rc, npulses = acquire_rc(gpu, out, geo, daq, dev, good, W_CUT, null_columns=True)
    assert rc == ERR_INVALID and npulses == SENTINEL, 'null outputs with a capacity'
    gpu.get_context().synchronize()
    out.assert_untouched('refused calls')
    # an empty photon window: nothing to do, and that is said in the outputs
    for bounds in ([300, 300], [0, 0, 0], [n, n]):
        rc, naccepted = count_rc(gpu, geo, daq, dev, bounds, W_CUT)
        assert rc == 0 and naccepted == 0
        empty = Outputs(len(bounds) - 1, 4)
        rc, npulses = acquire_rc(gpu, empty, geo, daq, dev, bounds, W_CUT)
        assert rc == 0 and npulses == 0
        got = empty.get()
        k = len(bounds) - 1
        assert (got['offsets'][:k + 1] == 0).all() and (got['offsets'][k + 1:] == SENTINEL).all()
        assert (got['outside'][:2 * k] == 0).all() and (got['outside'][2 * k:] == SENTINEL).all()
        assert all((got[name] == SENTINEL).all() for name in COLUMNS)
    # null pulse arrays with no capacity: the count alone (refused only if there IS a pulse)
    rc, npulses = acquire_rc(gpu, Outputs(1, 0), geo, daq, dev, [300, 300], W_CUT, null_columns=True)
    assert rc == 0 and npulses == 0
    # the end of the set itself is a bound like another
    rc, naccepted = count_rc(gpu, geo, daq, dev, [257, 300, 400, 500, n], W_ALL)
    _lib.check(rc)
    assert naccepted > 0


# ---- 7. through Simulation and chroma-sim ----------------------------------------------------------------------------------------
def bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def test_simulation_gives_every_event_its_pulses_beside_its_channels(gpu, tiny_geometry, tmp_path):
    """A few bomb events and an empty one through Simulation.simulate(run_daq=True) with and without daq_window, same seed:
    ev.channels is the same bit for bit; the pulses describe the same photoelectrons (earliest times, charges); chroma-sim
    --daq-window writes the arrays of ev.pulses."""
    from conftest import bomb, make_box_geometry
    from chroma_amd import cli
    from chroma_amd.gpu import tools
    from chroma_amd.sim import Simulation
    previous = tools._current
    window = (-8.0, 0.5, 512)          # 248 ns from the bomb on
    sizes = [400, 1, 3000, 64]
    try:
        runs = {}
        for with_window in (False, True):
            batch = [bomb(n, seed=300 + k) for k, n in enumerate(sizes)]
            batch.insert(2, event.Photons())
            sim = Simulation(tiny_geometry, seed=21)
            kw = dict(daq_window=window) if with_window else {}
            runs[with_window] = list(sim.simulate(batch, run_daq=True, max_steps=100, **kw))
            assert sim.gpu_daq.acquisition == len(batch)
            if with_window:
                with pytest.raises(ValueError):
                    list(sim.simulate(batch, daq_window=window))
                with pytest.raises(ValueError):
                    list(sim.simulate(batch, run_daq=True, daq_window=(0.0, 0.0, 5)))
                plain_geometry = Simulation(make_box_geometry(), seed=21)          # (no channels: no DAQ to bin)
                with pytest.raises(ValueError):
                    list(plain_geometry.simulate([bomb(10, seed=1)], run_daq=True, daq_window=window))
                del plain_geometry
            del sim
        unit = np.float32(tiny_geometry.charge_cdf[0][-1] / 2 ** 16)          # (the charge unit of GPUDaq)
        nchecked_t = nchecked_q = nlate = 0
        for plain, ev in zip(runs[False], runs[True]):
            assert plain.pulses is None and isinstance(ev.pulses, gpu.Pulses)
            for name in ('t', 'q', 'flags', 'hit'):
                assert np.array_equal(bits(getattr(ev.channels, name)), bits(getattr(plain.channels, name))), 'event %d: channels.%s' % (ev.id, name)
            p = ev.pulses
            nlate += p.late
            assert (np.diff(p.channel.astype(np.int64) * window[2] + p.bin) > 0).all()
            assert set(p.channel.tolist()) <= set(np.flatnonzero(ev.channels.flags != 0).tolist())
            assert np.array_equal(p.q.view(np.uint32), (p.q_int.astype(np.float32) * unit).astype(np.float32).view(np.uint32))
            assert len(p.bin_edges()) == window[2] + 1 and p.window == gpu.DaqWindow(*window)
            for channel in np.flatnonzero(ev.channels.hit):
                mine = p.channel == channel
                t = ev.channels.t[channel]
                if 0.0 <= t < 240.0:
                    # (the unsigned minimum of the channels skips negative times: t is the channel's earliest non-negative time,
                    #  and the window holds it, so it is the earliest of the channel's pulses from bin 16 = time 0 on)
                    mine = mine & (p.bin >= 16)
                    assert mine.any() and p.t_first[mine].min() == t, 'event %d, channel %d' % (ev.id, channel)
                    nchecked_t += 1
            if p.early == 0 and p.late == 0:
                # every accepted time of the event is in the window: the pulses of a channel hold its whole charge
                for channel in np.flatnonzero(ev.channels.flags != 0):
                    q = np.float32(p.q_int[p.channel == channel].sum(dtype=np.uint64).astype(np.uint32)) * unit
                    assert np.float32(q) == ev.channels.q[channel], 'event %d, channel %d' % (ev.id, channel)
                    nchecked_q += 1
                    npe, wq = p.waveform(channel)
                    assert npe.sum() == p.npe[p.channel == channel].sum() and npe.sum() >= 1
        print('channels checked: %d times, %d charges; late photons %d' % (nchecked_t, nchecked_q, nlate))
        assert len(runs[True][2].pulses) == 0 and nchecked_t > 20 and nchecked_q > 20
        # chroma-sim --daq-window: the arrays of ev.pulses, beside the channels of --run-daq
        files = {}
        for flag in ('--run-daq', '--daq-window'):
            files[flag] = str(tmp_path / (flag.strip('-') + '.npz'))
            argv = ['@chroma_amd.demo.tiny', '-n', '2', '--nphotons', '900', '-s', '4', '--max-steps', '100', '-o', files[flag]]
            assert cli.main(argv + ([flag] if flag == '--run-daq' else [flag + '=-8,0.5,512'])) == 0
        plain, binned = np.load(files['--run-daq']), np.load(files['--daq-window'])
        new = ['ev%d/pulse_%s' % (k, name) for k in range(2) for name in ('channel', 'bin', 'npe', 'q', 't', 'outside')]
        assert sorted(binned.files) == sorted(plain.files + new)
        daq_keys = [k for k in plain.files if '/daq_' in k]
        assert len(daq_keys) == 2 * 3
        for k in daq_keys:          # (the flat hits of a channel come in the order of an atomic: not compared)
            assert np.array_equal(bits(plain[k]), bits(binned[k])), k
        sim = Simulation(tiny_geometry, seed=4)
        rng = np.random.default_rng(sim.seed)
        events = list(sim.simulate([cli.bomb_event(900, 400.0, [0.0, 0.0, 0.0], rng) for _ in range(2)], keep_hits=False, run_daq=True,
                                   max_steps=100, daq_window=window))
        for k, ev in enumerate(events):
            p = ev.pulses
            for name, want in (('channel', p.channel), ('bin', p.bin), ('npe', p.npe), ('q', p.q), ('t', p.t_first),
                               ('outside', np.array([p.early, p.late], dtype=np.uint32))):
                got = binned['ev%d/pulse_%s' % (k, name)]
                assert got.dtype == want.dtype and np.array_equal(bits(got), bits(want)), 'ev%d/pulse_%s' % (k, name)
            assert len(p) > 0
        del sim
    finally:
        tools._current = previous
