"""The trigger of the time-binned DAQ on the GPU -- chroma_daq_trigger_pulses (k_daq_trigger_edges / _count / _fire / _gates /
_compact / _reduce around hipCUB's scans and sort and the pulse kernels' heads / open / finish), GPUEventDaq.acquire_pulses(
trigger=...) and Simulation.simulate(daq_trigger=...) over it -- bit for bit on the brute-force restatement of
tests/test_daq_trigger_host.py, on that module's pulse sets (uploaded as they are: the trigger is a function of the pulse arrays)
and on the pulses the library itself acquires.  Every output array is longer than what the call may write and pre-filled with a
sentinel, which the words beyond must still hold.
"""
import ctypes

import numpy as np
import pytest

from chroma_amd import event
from test_gpu_photon_arrays import geos, host_geos, gpu, upload, DAQ_BASE, SENTINEL, GUARD_WORDS      # noqa: F401
from test_gpu_daq_events import tables_of, BASE, WEIGHT, ERR_INVALID
from test_daq_pulses_host import restated, expected_pulses, W_ALL, W_CUT, SEED          # noqa: F401
from test_gpu_daq_pulses import Outputs as PulseOutputs, acquire_rc
from test_daq_trigger_host import cases, brute, brute_of, from_rows, PulseSet, NAMES, NONE, bits, as_dict, assert_same

pytestmark = pytest.mark.gpu

KINDS = {'nhit': 0, 'npe': 1}
WINDOW = (-8.0, 0.5)          # (t0, dt): the trigger works in bins


class Outputs(object):
    """The device outputs of one chroma_daq_trigger_pulses call, sentinel-filled: trig_offsets (nrows + 1), trig_bin and trig_sum
    (trigger_capacity), hit_offsets (trigger_capacity + 1), the five hit arrays (hit_capacity), pulse_trigger (npulses),
    GUARD_WORDS more each."""

    def __init__(self, nrows, npulses, trigger_capacity, hit_capacity):
        from chroma_amd.gpu.tools import to_gpu
        self.sizes = dict(trig_offsets=nrows + 1, trig_bin=trigger_capacity, trig_sum=trigger_capacity, hit_offsets=trigger_capacity + 1,
                          hit_channel=hit_capacity, hit_npe=hit_capacity, hit_q_int=hit_capacity, hit_t_first=hit_capacity, hit_flags=hit_capacity,
                          pulse_trigger=npulses)
        self.arrays = {name: to_gpu(np.full(self.sizes[name] + GUARD_WORDS, SENTINEL, dtype=np.uint32)) for name in NAMES}
        self.trigger_capacity, self.hit_capacity = trigger_capacity, hit_capacity

    def get(self):
        return {name: a.get() for name, a in self.arrays.items()}

    def assert_untouched(self, what):
        for name, a in self.get().items():
            assert (a == SENTINEL).all(), '%s: %s was written' % (what, name)


class Device(object):
    """A PulseSet on the device."""

    def __init__(self, ps):
        from chroma_amd.gpu.tools import to_gpu
        self.ps = ps
        self.offsets = to_gpu(ps.offsets)
        self.columns = [to_gpu(a) for a in ps.columns()]


def trigger_rc(gpu, dev, out, kind, trig, nbins=None, nrows=None, nchannels=None, null=(), no_pulse_trigger=False, dt=WINDOW[1], npulses=None):
    from chroma_amd import _lib
    ps = dev.ps
    ctx = gpu.get_context()
    win = _lib.DaqWindow(WINDOW[0], dt, ps.nbins if nbins is None else nbins)
    t = _lib.DaqTrigger(KINDS.get(kind, kind), *trig)
    a = {name: (None if name in null else arr.ptr) for name, arr in out.arrays.items()}
    inputs = [None if 'inputs' in null else arr.ptr for arr in dev.columns]
    ntriggers, nhits = ctypes.c_uint64(SENTINEL), ctypes.c_uint64(SENTINEL)
    rc = ctx._lib.chroma_daq_trigger_pulses(
        ctx.handle, ps.nrows if nrows is None else nrows, ps.nchannels if nchannels is None else nchannels, ctypes.byref(win), ctypes.byref(t),
        None if 'offsets' in null else dev.offsets.ptr, *(inputs + [len(ps) if npulses is None else npulses, out.trigger_capacity, a['trig_offsets'],
                                                                    a['trig_bin'], a['trig_sum'], a['hit_offsets'], out.hit_capacity, a['hit_channel'], a['hit_npe'], a['hit_q_int'],
                                                                    a['hit_t_first'], a['hit_flags'], None if no_pulse_trigger else a['pulse_trigger'],
                                                                    ctypes.byref(ntriggers), ctypes.byref(nhits)]))
    return rc, int(ntriggers.value), int(nhits.value)


def assert_triggers(out, ntriggers, nhits, want, what):
    got = out.get()
    nt, nh = len(want['trig_bin']), len(want['hit_channel'])
    assert (ntriggers, nhits) == (nt, nh), '%s: %d triggers and %d hits, expected %d and %d' % (what, ntriggers, nhits, nt, nh)
    written = dict(out.sizes, trig_bin=nt, trig_sum=nt, hit_offsets=nt + 1, hit_channel=nh, hit_npe=nh, hit_q_int=nh, hit_t_first=nh, hit_flags=nh)
    for name in NAMES:
        n = written[name]
        assert np.array_equal(got[name][:n], bits(want[name]).view(np.uint32)), '%s: %s\n%s\n%s' % (what, name, got[name][:n], want[name])
        assert (got[name][n:] == SENTINEL).all() and len(got[name]) == out.sizes[name] + GUARD_WORDS, '%s: words behind %s' % (what, name)


def run_exact(gpu, ps, kind, trig, want, what):
    """The call with exactly the capacities the restatement needs."""
    from chroma_amd import _lib
    out = Outputs(ps.nrows, len(ps), len(want['trig_bin']), len(want['hit_channel']))
    rc, ntriggers, nhits = trigger_rc(gpu, Device(ps), out, kind, trig)
    _lib.check(rc)
    assert_triggers(out, ntriggers, nhits, want, what)


# ---- 1. the call is the restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['nhit', 'npe'])
def test_the_call_is_the_restatement_on_the_synthetic_pulse_sets(gpu, kind):
    for index, (name, ps, trig) in enumerate(cases()):
        run_exact(gpu, ps, kind, trig, brute(index, kind), '%s, %s' % (name, kind))


def more_sets():
    rng = np.random.default_rng(77)
    # 300 rows of one bin each: more rows than lanes in a wave, blocks in which the row changes at every pulse (some rows empty,
    # some with two or three channels)
    rows = [{(int(c), 0) for c in rng.permutation(4)[:rng.integers(0, 4)]} for _ in range(300)]
    yield '300 rows of one bin', from_rows(300, 4, 1, rows, rng), (2, 1, 1, 0, 1)
    # 2000 pulses in one row: eight blocks of one row, runs of a channel over many bins, many lanes onto one (row, bin) word
    pairs = rng.permutation(50 * 64)[:2000]
    yield '2000 pulses in one row', from_rows(1, 50, 64, [{(int(p // 64), int(p % 64)) for p in pairs}], rng), (33, 2, 5, 1, 3)


@pytest.mark.parametrize('kind', ['nhit', 'npe'])
def test_many_rows_of_one_bin_and_one_row_of_many_pulses(gpu, kind):
    for name, ps, trig in more_sets():
        want = brute_of(ps, kind, *trig)
        per_row = np.diff(want['trig_offsets'].astype(np.int64))
        assert per_row.max() >= 1 and (ps.nrows == 1 or per_row.min() == 0), name
        run_exact(gpu, ps, kind, trig, want, '%s, %s' % (name, kind))


def test_no_pulse_is_no_trigger(gpu):
    ps = PulseSet(5, 3, 40, np.zeros(6), [], [], [], [], [], [])
    for null in ((), ('inputs',)):
        out = Outputs(5, 0, 2, 2)
        rc, ntriggers, nhits = trigger_rc(gpu, Device(ps), out, 'nhit', (1, 1, 1, 0, 1), null=null)
        assert (rc, ntriggers, nhits) == (0, 0, 0)
        got = out.get()
        assert (got['trig_offsets'][:6] == 0).all() and (got['trig_offsets'][6:] == SENTINEL).all()
        assert got['hit_offsets'][0] == 0 and (got['hit_offsets'][1:] == SENTINEL).all()
        assert all((got[name] == SENTINEL).all() for name in NAMES if name not in ('trig_offsets', 'hit_offsets'))


# ---- 2. capacities --------------------------------------------------------------------------------------------------------------------------
def test_a_capacity_one_short_is_refused_with_the_counts(gpu):
    from chroma_amd import _lib
    index = 1
    name, ps, trig = cases()[index]
    want = brute(index, 'nhit')
    nt, nh = len(want['trig_bin']), len(want['hit_channel'])
    assert nt > 2 and nh > nt
    dev = Device(ps)
    for short_t, short_h in ((1, 0), (0, 1)):
        out = Outputs(ps.nrows, len(ps), nt - short_t, nh - short_h)
        rc, ntriggers, nhits = trigger_rc(gpu, dev, out, 'nhit', trig)
        assert rc == ERR_INVALID and (ntriggers, nhits) == (nt, nh)
        gpu.get_context().synchronize()
        out.assert_untouched('capacities %d of %d and %d of %d' % (nt - short_t, nt, nh - short_h, nh))
    out = Outputs(ps.nrows, len(ps), nt, nh)
    rc, ntriggers, nhits = trigger_rc(gpu, dev, out, 'nhit', trig)
    _lib.check(rc)
    assert_triggers(out, ntriggers, nhits, want, 'capacities == need')
    # without the per-pulse array: the rest is the same
    out = Outputs(ps.nrows, len(ps), nt + 3, nh + 5)
    rc, ntriggers, nhits = trigger_rc(gpu, dev, out, 'nhit', trig, no_pulse_trigger=True)
    _lib.check(rc)
    assert_triggers(out, ntriggers, nhits, dict(want, pulse_trigger=np.full(len(ps), SENTINEL, dtype=np.uint32)), 'no pulse_trigger')
    # the bound of the header suffices
    threshold, W, H, pre, post = trig
    bound = min(ps.nrows * -(-ps.nbins // H), len(ps) * -(-W // H))
    assert nt <= bound and nh <= len(ps)


# ---- 3. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_bad_triggers_windows_and_arrays_are_refused_before_anything_is_launched(gpu):
    name, ps, trig = cases()[0]          # (70 bins; threshold 3, W 4, H 6, pre 2, post 4)
    dev = Device(ps)
    out = Outputs(ps.nrows, len(ps), 64, len(ps))
    refused = [('threshold 0', dict(trig=(0, 4, 6, 2, 4))), ('width 0', dict(trig=(3, 0, 6, 2, 4))), ('width beyond the window', dict(trig=(3, 71, 80, 2, 4))),
               ('post 0', dict(trig=(3, 4, 6, 2, 0))), ('holdoff below pre + post', dict(trig=(3, 4, 5, 2, 4))), ('holdoff 0', dict(trig=(3, 4, 0, 0, 1))),
               ('pre + post beyond 32 bits', dict(trig=(3, 4, 6, 0xffffffff, 8))), ('an unknown kind', dict(trig=trig, kind=2)),
               ('no bins', dict(trig=trig, nbins=0)), ('65537 bins', dict(trig=trig, nbins=65537)), ('dt 0', dict(trig=trig, dt=0.0)),
               ('dt NaN', dict(trig=trig, dt=float('nan'))), ('no rows', dict(trig=trig, nrows=0)), ('no channels', dict(trig=trig, nchannels=0)),
               ('2^32 pulses', dict(trig=trig, npulses=1 << 32)), ('no offsets', dict(trig=trig, null=('offsets',))),
               ('no pulse arrays', dict(trig=trig, null=('inputs',))), ('no trigger offsets', dict(trig=trig, null=('trig_offsets',))),
               ('no hit offsets', dict(trig=trig, null=('hit_offsets',))), ('no trigger bins', dict(trig=trig, null=('trig_bin',))),
               ('no hit flags', dict(trig=trig, null=('hit_flags',)))]
    for what, kw in refused:
        kw.setdefault('kind', 'nhit')
        rc, ntriggers, nhits = trigger_rc(gpu, dev, out, kw.pop('kind'), kw.pop('trig'), **kw)
        assert rc == ERR_INVALID, what
    gpu.get_context().synchronize()
    out.assert_untouched('refused calls')


# ---- 4. entries that count for nothing ----------------------------------------------------------------------------------------------------------
def test_a_bin_behind_the_window_and_channels_outside_the_detector_count_for_nothing(gpu):
    """A sorted set to which a bin equal to nbins (behind the bins of its channel), a channel equal to nchannels (behind its row) and
    a channel of -1 (before its row) are added -- the arrays stay ordered, and every index the kernels form from them stays
    within the arrays of this test: the output is that of the set without them, and their pulse_trigger says none."""
    from chroma_amd import _lib
    index = 0
    name, ps, trig = cases()[index]
    want = brute(index, 'nhit')
    nch, nbins = ps.nchannels, ps.nbins
    columns = [list(a) for a in ps.columns()]
    added, offsets = [], [0]
    out_columns = [[] for _ in columns]
    for r in range(ps.nrows):
        lo, hi = int(ps.offsets[r]), int(ps.offsets[r + 1])
        entries = [tuple(c[i] for c in columns) + (False,) for i in range(lo, hi)]
        if r in (0, 3, ps.nrows - 1) and hi > lo:
            c0 = entries[0][0]
            last_of_c0 = max(i for i, e in enumerate(entries) if e[0] == c0)
            entries.insert(last_of_c0 + 1, (c0, nbins, 3, 77, np.float32(-50.0), 0x800, True))
            entries.append((nch, 5, 3, 77, np.float32(-50.0), 0x800, True))
            entries.insert(0, (-1, 5, 3, 77, np.float32(-50.0), 0x800, True))
        for e in entries:
            for k in range(6):
                out_columns[k].append(e[k])
            added.append(e[6])
        offsets.append(len(added))
    added = np.array(added)
    assert added.sum() == 9
    bad = PulseSet(ps.nrows, nch, nbins, offsets, *out_columns)
    key = (np.repeat(np.arange(ps.nrows), np.diff(bad.offsets.astype(np.int64))) * (nch + 2) + bad.channel.astype(np.int64) + 1) * (nbins + 1) + bad.bin
    assert (np.diff(key) > 0).all()          # (still in (row, channel, bin) order)
    pulse_trigger = np.full(len(bad), NONE, dtype=np.uint32)
    pulse_trigger[~added] = want['pulse_trigger']
    for kind in ('nhit', 'npe'):
        w = brute(index, kind)
        of = np.full(len(bad), NONE, dtype=np.uint32)
        of[~added] = w['pulse_trigger']
        out = Outputs(bad.nrows, len(bad), len(w['trig_bin']), len(w['hit_channel']))
        rc, ntriggers, nhits = trigger_rc(gpu, Device(bad), out, kind, trig)
        _lib.check(rc)
        assert_triggers(out, ntriggers, nhits, dict(w, pulse_trigger=of), 'with entries that count for nothing, ' + kind)


# ---- 5. on the pulses the library acquires ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', ['tiny', 'stress'])
def test_the_trigger_on_acquired_pulses_is_the_restatement_on_the_restated_pulses(gpu, geos, restated, which):
    from chroma_amd import _lib
    from chroma_amd.gpu.tools import to_gpu
    geo = geos[which]
    rows, bounds, acc = restated(which)
    nrows = len(bounds) - 1
    daq = tables_of(gpu, geo)
    dev = upload(rows)
    for window, (W, H, pre, post) in ((W_ALL, (8, 24, 4, 20)), (W_CUT, (2, 2, 0, 2))):
        pulses = expected_pulses(acc, window, nrows, geo.nchannels)
        ps = PulseSet(nrows, geo.nchannels, window[2], pulses['offsets'], pulses['channel'], pulses['bin'], pulses['npe'], pulses['q_int'],
                      pulses['t_first'].view(np.float32), pulses['flags'])
        acquired = PulseOutputs(nrows, pulses['naccepted'])
        rc, npulses = acquire_rc(gpu, acquired, geo, daq, dev, bounds, window)
        _lib.check(rc)
        assert npulses == len(ps) > 0
        on_device = Device.__new__(Device)
        on_device.ps, on_device.offsets, on_device.columns = ps, acquired.offsets, acquired.columns
        for kind in ('nhit', 'npe'):
            # the threshold from the restated pulses: the highest of these at which any row fires (empty rows never do)
            for threshold in (12, 6, 4, 3, 2, 1):
                want = brute_of(ps, kind, threshold, W, H, pre, post)
                if len(want['trig_bin']):
                    break
            per_row = np.diff(want['trig_offsets'].astype(np.int64))
            what = '%s, window %s, %s >= %d' % (which, window, kind, threshold)
            assert (per_row > 0).any() and (per_row == 0).any(), what
            out = Outputs(nrows, len(ps), len(want['trig_bin']), len(want['hit_channel']))
            rc, ntriggers, nhits = trigger_rc(gpu, on_device, out, kind, (threshold, W, H, pre, post))
            _lib.check(rc)
            assert_triggers(out, ntriggers, nhits, want, what)


# ---- 6. GPUEventDaq.acquire_pulses(trigger=...) ---------------------------------------------------------------------------------------------------
def test_acquire_pulses_with_a_trigger_does_not_depend_on_the_chunking_and_is_the_host_twin(gpu, geos, restated):
    from chroma_amd import _lib
    geo = geos['tiny']
    rows, bounds, acc = restated('tiny', 'many')
    nrows = len(bounds) - 1
    dev = upload(rows)
    trigger = gpu.DaqTrigger(1, 4, 8, 2, 6)
    results = {}
    for rows_per_chunk in (7, None):
        event_daq = gpu.GPUEventDaq(geo.gg) if rows_per_chunk is None else gpu.GPUEventDaq(geo.gg, max_entries=7 * geo.nchannels + geo.nchannels - 1)
        assert event_daq.rows_per_chunk == (rows_per_chunk or event_daq.rows_per_chunk) and (rows_per_chunk or event_daq.rows_per_chunk >= nrows)
        rng = _lib.Rng(SEED, DAQ_BASE)
        channels_before = event_daq.acquire(dev, rng, bounds, acquisition=BASE, weight=WEIGHT)
        plain = event_daq.acquire_pulses(dev, rng, bounds, W_ALL, acquisition=BASE, weight=WEIGHT)
        pulses = event_daq.acquire_pulses(dev, rng, bounds, W_ALL, acquisition=BASE, weight=WEIGHT, trigger=trigger)
        channels_after = event_daq.acquire(dev, rng, bounds, acquisition=BASE, weight=WEIGHT)
        assert plain.triggers is None and isinstance(pulses.triggers, gpu.EventTriggers) and len(pulses.triggers) == nrows
        for name in ('offsets', 'channel', 'bin', 'npe', 'q_int', 't_first', 'flags', 'q'):
            assert np.array_equal(bits(getattr(pulses, name)), bits(getattr(plain, name))), name
        for r in (0, 7, 8, nrows - 1):
            for a, b in zip(channels_before.sparse(r), channels_after.sparse(r)):
                assert np.array_equal(bits(a), bits(b))
        assert_same(as_dict(pulses.triggers), as_dict(pulses.trigger(trigger)), '%s rows per chunk against the host' % rows_per_chunk)
        results[rows_per_chunk] = pulses.triggers
    assert_same(as_dict(results[7]), as_dict(results[None]), 'chunks of 7 rows against one chunk')
    per_row = np.diff(results[7].offsets)
    assert (per_row > 0).sum() > 100 and (per_row == 0).sum() > 100
    r = int(np.argmax(per_row))
    t = results[7].event(r)
    assert isinstance(t, gpu.Triggers) and len(t) == per_row[r] and len(t.pulse_trigger) == len(pulses.event(r))
    assert isinstance(t.channels(0), event.Channels) and t.channels(0).hit.sum() == len(t.sparse(0)[0]) - (t.sparse(0)[3] >= 1e8).sum()


# ---- 7. through Simulation and chroma-sim ------------------------------------------------------------------------------------------------------------
def test_simulation_gives_every_event_its_triggers_and_nothing_else_changes(gpu, tiny_geometry, tmp_path):
    from conftest import bomb
    from chroma_amd import cli
    from chroma_amd.gpu import tools
    from chroma_amd.sim import Simulation
    previous = tools._current
    window = (-8.0, 0.5, 512)
    trigger = (2, 16, 64, 8, 40)
    sizes = [400, 1, 3000, 64]
    try:
        runs = {}
        for with_trigger in (False, True):
            batch = [bomb(n, seed=300 + k) for k, n in enumerate(sizes)]
            batch.insert(2, event.Photons())
            sim = Simulation(tiny_geometry, seed=21)
            kw = dict(daq_trigger=trigger) if with_trigger else {}
            runs[with_trigger] = list(sim.simulate(batch, run_daq=True, max_steps=100, daq_window=window, **kw))
            if with_trigger:
                with pytest.raises(ValueError):
                    list(sim.simulate(batch, run_daq=True, daq_trigger=trigger))
                with pytest.raises(ValueError):
                    list(sim.simulate(batch, run_daq=True, daq_window=window, daq_trigger=(2, 513)))
            del sim
        nfired = 0
        for plain, ev in zip(runs[False], runs[True]):
            assert plain.triggers is None and isinstance(ev.triggers, gpu.Triggers)
            for name in ('t', 'q', 'flags', 'hit'):
                assert np.array_equal(bits(getattr(ev.channels, name)), bits(getattr(plain.channels, name))), 'event %d: channels.%s' % (ev.id, name)
            for name in ('channel', 'bin', 'npe', 'q_int', 't_first', 'flags'):
                assert np.array_equal(bits(getattr(ev.pulses, name)), bits(getattr(plain.pulses, name))), 'event %d: pulses.%s' % (ev.id, name)
            order = lambda h: np.lexsort((h.wavelengths.view(np.uint32), h.t.view(np.uint32), h.channel))
            assert len(ev.flat_hits) == len(plain.flat_hits)
            for name in ('channel', 't', 'wavelengths', 'flags'):          # (the flat hits of a channel come in the order of an atomic)
                assert np.array_equal(bits(getattr(ev.flat_hits, name))[order(ev.flat_hits)], bits(getattr(plain.flat_hits, name))[order(plain.flat_hits)])
            # ev.triggers is ev.pulses triggered on the host
            p = ev.pulses
            alone = gpu.EventPulses(p.window, p.nchannels, 1.0, np.array([0, len(p)], dtype=np.int64), p.channel, p.bin, p.npe, p.q_int, p.t_first,
                                    p.flags, outside=np.zeros((1, 2), dtype=np.uint32))
            want = alone.trigger(trigger).event(0)
            t = ev.triggers
            for name in ('bin', 'sum', 'hit_offsets', 'hit_channel', 'hit_npe', 'hit_q_int', 'hit_t_first', 'hit_flags', 'pulse_trigger'):
                assert np.array_equal(bits(getattr(t, name)), bits(getattr(want, name))), 'event %d: triggers.%s' % (ev.id, name)
            assert np.array_equal(t.time, window[0] + window[1] * t.bin.astype(np.float64))
            nfired += len(t)
        print('triggers per event:', [len(ev.triggers) for ev in runs[True]])
        assert nfired >= 1 and len(runs[True][1].triggers) == 0 and len(runs[True][2].triggers) == 0 and len(runs[True][3].triggers) >= 1
        # chroma-sim --daq-trigger: the arrays of ev.triggers beside those of --daq-window
        files = {}
        for flag in ('window', 'trigger'):
            files[flag] = str(tmp_path / (flag + '.npz'))
            argv = ['@chroma_amd.demo.tiny', '-n', '2', '--nphotons', '900', '-s', '4', '--max-steps', '100', '-o', files[flag], '--daq-window=-8,0.5,512']
            assert cli.main(argv + (['--daq-trigger', '2,16,64,8,40'] if flag == 'trigger' else [])) == 0
        binned, triggered = np.load(files['window']), np.load(files['trigger'])
        names = ('trigger_bin', 'trigger_time', 'trigger_sum', 'trigger_hit_offsets', 'trigger_hit_channel', 'trigger_hit_npe', 'trigger_hit_q',
                 'trigger_hit_t', 'pulse_trigger')
        assert sorted(triggered.files) == sorted(binned.files + ['ev%d/%s' % (k, name) for k in range(2) for name in names])
        for k in binned.files:
            if '/daq_' in k or '/pulse_' in k:
                assert np.array_equal(bits(binned[k]), bits(triggered[k])), k
        sim = Simulation(tiny_geometry, seed=4)
        rng = np.random.default_rng(sim.seed)
        events = list(sim.simulate([cli.bomb_event(900, 400.0, [0.0, 0.0, 0.0], rng) for _ in range(2)], keep_hits=False, run_daq=True,
                                   max_steps=100, daq_window=window, daq_trigger=trigger))
        for k, ev in enumerate(events):
            t = ev.triggers
            for name, want in (('trigger_bin', t.bin), ('trigger_time', t.time), ('trigger_sum', t.sum), ('trigger_hit_offsets', t.hit_offsets),
                               ('trigger_hit_channel', t.hit_channel), ('trigger_hit_npe', t.hit_npe), ('trigger_hit_q', t.hit_q),
                               ('trigger_hit_t', t.hit_t_first), ('pulse_trigger', t.pulse_trigger)):
                got = triggered['ev%d/%s' % (k, name)]
                assert got.dtype == want.dtype and np.array_equal(bits(got), bits(want)), 'ev%d/%s' % (k, name)
        assert sum(len(ev.triggers) for ev in events) >= 1
        del sim
    finally:
        tools._current = previous
