"""The batch DAQ -- chroma_daq_acquire_events (k_run_daq_events), chroma_daq_compact_events (k_daq_events_flag, a scan,
k_daq_events_scatter), GPUEventDaq / EventChannels and Simulation.simulate(run_daq=True) over them -- bit for bit on the CPU
oracle's run_daq called once per event: row r of a batch is the oracle's acquisition ``base + r`` of the photons
[bounds[r], bounds[r + 1]) onto a fresh state.

The photons are those of the DAQ tests of test_gpu_photon_arrays.py (``daq_rows``: per-photon weights in [0, 1] under the
global weight 0.7, a photon id base beyond 2^32, guard photons around the window that sit on the dark channels with weight 1
and would fire them).  The events (``event_bounds``) start at photon 257 and end below the end of the set, with empty events
first, in the middle and last, runs of single-photon events, events that straddle a multiple of 64 and of 256 -- of the photon
index and of its distance from the first bound, which is what the kernel's waves and blocks are cut by -- and one event longer
than a block of 256.  The second set (``many_bounds``) is some 1300 events of zero to three photons: more than 2^16 + 257
(row, channel) words, so that the compaction's scan runs over several tiles, and rows_per_chunk 1 and 7 cut it into many chunks.
"""
import ctypes

import numpy as np
import pytest

from chroma_amd import event
from test_gpu_photon_arrays import (geos, host_geos, gpu, upload, windowed, daq_rows, daq_tables, assert_channels, DAQ_BASE,      # noqa: F401
                                    DAQ_FIRST, DAQ_N, DETECT, SENTINEL, GUARD_WORDS, call, structure)

gpu_test = pytest.mark.gpu

BASE = 5                            # the acquisition number of row 0
WEIGHT = 0.7
RESET_BITS = int(np.float32(1e9).view(np.uint32))
ERR_INVALID = -1                    # CHROMA_ERR_INVALID


# ---- the events ------------------------------------------------------------------------------------------------------------
def event_bounds():
    """38 events over the window [DAQ_FIRST, DAQ_FIRST + DAQ_N) of ``daq_rows``."""
    sizes = [0, 0, 1, 1, 1, 1, 1, 37, 0, 0, 120, 1, 1, 1, 64, 200, 0, 700, 1, 1, 3, 256, 2, 0, 333, 1, 1, 1, 1, 90, 0, 5, 17, 1, 250]
    sizes += [DAQ_N - sum(sizes), 0, 0]
    bounds = DAQ_FIRST + np.cumsum([0] + sizes)
    assert bounds[0] == 257 and bounds[-1] == DAQ_FIRST + DAQ_N and (np.diff(bounds) >= 0).all()
    return bounds.astype(np.uint32)


def many_rows_and_bounds(geo):
    """(rows, bounds) of the compaction tests: a copy of ``daq_rows`` and some 1300 events of zero to three photons over it, the
    first and the last of three photons.  Those six photons carry the detection flag and weight 1, the first three on channel 0,
    the last three on the last channel: the first and the last word of the state are touched if the gate lets one of three
    through (the twin test checks that it does)."""
    nrows = max(1300, -(-(2 ** 16 + 258) // geo.nchannels))
    rng = np.random.default_rng(77)
    sizes = rng.integers(0, 4, nrows)
    sizes[0] = sizes[-1] = 3
    bounds = (DAQ_FIRST + np.cumsum(np.concatenate([[0], sizes]))).astype(np.uint32)
    assert bounds[-1] < DAQ_FIRST + DAQ_N and nrows * geo.nchannels > 2 ** 16 + 257
    rows = daq_rows(geo, seed=62)
    ph = rows[0]
    for where, channel in ((slice(int(bounds[0]), int(bounds[1])), 0), (slice(int(bounds[-2]), int(bounds[-1])), geo.nchannels - 1)):
        triangles = geo.triangles_of([channel])
        assert len(triangles)
        ph.last_hit_triangles[where] = triangles[0]
        ph.flags[where] |= np.uint32(DETECT)
        ph.weights[where] = 1.0
    return rows, bounds


def oracle_rows(oracle_mod, geo, ph, bounds, base=BASE, stride=None, acquires=1):
    """The stacked state (time bits, charge counts, histories; nrows * stride words each) of the oracle's run_daq called once
    per row onto that row's words of a fresh state; ``acquires`` > 1: again with the acquisitions numbered on, no reset."""
    stride = geo.nchannels if stride is None else stride
    nrows = len(bounds) - 1
    tables, unit = daq_tables(geo)
    state = oracle_mod.daq_state(nrows * stride)
    for k in range(acquires):
        for r in range(nrows):
            words = tuple(a[r * stride:(r + 1) * stride] for a in state)
            oracle_mod.run_daq(geo.packed, ph, tables, unit, seed=9, photon_id_base=DAQ_BASE, acquisition=base + k * nrows + r, weight=WEIGHT,
                               start_photon=int(bounds[r]), nphotons=int(bounds[r + 1]) - int(bounds[r]), state=words)
    for a in state:
        a.flags.writeable = False
    return state


@pytest.fixture(scope='module')
def expected(oracle_mod, host_geos):
    """The oracle's stacked states, computed once per case and shared read-only: expected(which, kind) -> (rows, bounds, state)."""
    cache = {}

    def get(which, kind='events', **kw):
        key = (which, kind) + tuple(sorted(kw.items()))
        if key not in cache:
            geo = host_geos[which]
            rows, bounds = (daq_rows(geo), event_bounds()) if kind == 'events' else many_rows_and_bounds(geo)
            cache[key] = (rows, bounds, oracle_rows(oracle_mod, geo, rows[0], bounds, **kw))
        return cache[key]
    return get


def row_channels(geo, state, r, stride=None):
    """(t, q, flags, hit) of row r of a stacked state, as GPUChannels.get() gives them."""
    stride = geo.nchannels if stride is None else stride
    w = slice(r * stride, r * stride + geo.nchannels)
    t = state[0][w].view(np.float32)
    q = (state[1][w].astype(np.float32) * np.float32(daq_tables(geo)[1])).astype(np.float32)
    return t, q, state[2][w], t < 1e8


# ---- the calls -------------------------------------------------------------------------------------------------------------
def tables_of(gpu, geo):
    """The chroma_daq_tables of a detector (and the object that keeps their device arrays alive)."""
    daq = gpu.GPUDaq(geo.gg)
    daq_tables(geo, daq)
    return daq


def device_state(gpu, words, fill=SENTINEL):
    from chroma_amd.gpu.tools import to_gpu
    return [to_gpu(np.full(words + GUARD_WORDS, fill, dtype=np.uint32)) for _ in range(3)]


def acquire_events_rc(gpu, geo, daq, dev, bounds, arrays, nrows=None, acquisition=BASE, stride=None, nphotons=None):
    from chroma_amd import _lib
    ctx = gpu.get_context()
    bounds = np.ascontiguousarray(bounds, dtype=np.uint32)
    s = structure(dev)
    return ctx._lib.chroma_daq_acquire_events(ctx.handle, geo.gg.handle, ctypes.byref(daq.tables), len(bounds) - 1 if nrows is None else nrows,
                                              _lib.ptr(bounds), DETECT, ctypes.byref(s), len(dev.pos) if nphotons is None else nphotons,
                                              _lib.Rng(9, DAQ_BASE), acquisition, WEIGHT, geo.nchannels if stride is None else stride,
                                              arrays[0].ptr, arrays[1].ptr, arrays[2].ptr)


def acquire_events(*args, **kw):
    from chroma_amd import _lib
    _lib.check(acquire_events_rc(*args, **kw))


def assert_state(arrays, state, words, what):
    for got, want, name in zip(arrays, state, ('time bits', 'charge counts', 'histories')):
        got = got.get()
        assert np.array_equal(got[:words], want), '%s: %s' % (what, name)
        assert (got[words:] == SENTINEL).all(), '%s: guard words behind the %s' % (what, name)


def compact(gpu, geo, arrays, nrows, capacity, unit, stride=None):
    from chroma_amd.gpu.tools import to_gpu
    out = [to_gpu(np.full(nrows + 1 + GUARD_WORDS, SENTINEL, dtype=np.uint32))]
    out += [to_gpu(np.full(capacity + GUARD_WORDS, SENTINEL, dtype=np.uint32).view(dtype)) for dtype in (np.int32, np.float32, np.float32, np.uint32)]
    ntouched = ctypes.c_uint64(0)
    call(gpu, 'chroma_daq_compact_events', nrows, geo.nchannels, geo.nchannels if stride is None else stride, unit, arrays[0].ptr, arrays[1].ptr,
         arrays[2].ptr, capacity, *[a.ptr for a in out], ctypes.byref(ntouched))
    return int(ntouched.value), [a.get() for a in out]


def expected_sparse(geo, state, nrows, stride=None):
    """(offsets, channel, time bits, q, flags) of the touched words of a stacked state in row-major order."""
    stride = geo.nchannels if stride is None else stride
    hist = state[2].reshape(nrows, stride)[:, :geo.nchannels]
    row, channel = np.nonzero(hist)
    word = row * stride + channel
    offsets = np.concatenate([[0], np.cumsum((hist != 0).sum(axis=1))]).astype(np.uint32)
    q = (state[1][word].astype(np.float32) * np.float32(daq_tables(geo)[1])).astype(np.float32)
    return offsets, channel.astype(np.int32), state[0][word], q, state[2][word]


def assert_sparse(got, ntouched, want, nrows, capacity, what):
    offsets, channel, t, q, flags = want
    assert ntouched == len(channel) == offsets[-1], what
    assert np.array_equal(got[0][:nrows + 1], offsets), what + ': offsets'
    assert np.array_equal(got[1][:ntouched], channel), what + ': channel'
    assert np.array_equal(got[2][:ntouched].view(np.uint32), t), what + ': t'
    assert np.array_equal(got[3][:ntouched].view(np.uint32), q.view(np.uint32)), what + ': q'
    assert np.array_equal(got[4][:ntouched], flags), what + ': flags'
    assert (got[0][nrows + 1:] == SENTINEL).all(), what + ': guard words behind the offsets'
    for a in got[1:]:
        assert (a.view(np.uint32)[ntouched:] == SENTINEL).all() and len(a) == capacity + GUARD_WORDS, what + ': words behind the touched ones'


# ---- without a GPU: the inputs do their job --------------------------------------------------------------------------------
@pytest.mark.parametrize('which', ['tiny', 'stress'])
def test_event_inputs_exercise_shared_words_timeless_words_empty_rows_and_block_edges(oracle_mod, host_geos, expected, which):
    """From the oracle's output alone: a row with two or more touched channels, a word with more charge than one photon can
    add, a word with a history and a charge but no time (more than one channel only), an empty event between two that touched
    something, an event whose photons cross a multiple of 256 (and of 64; of the index and of the distance from the first
    bound alike), one longer than a block, runs of single-photon events; and the guard photons, inside a window, fire channels
    that stay dark in every row."""
    geo = host_geos[which]
    rows, bounds, state = expected(which)
    nrows, nch = len(bounds) - 1, geo.nchannels
    assert bounds[0] == 257 and bounds[-1] < len(rows[0]) and 35 <= nrows <= 45
    hist = state[2].reshape(nrows, nch)
    q = state[1].reshape(nrows, nch).astype(np.float32) * np.float32(daq_tables(geo)[1])
    timeless = (hist != 0) & (state[0].reshape(nrows, nch) == RESET_BITS)
    one_photon_most = np.float32(daq_tables(geo)[0][2][-1]) * np.float32(1.01)
    assert (q > one_photon_most).any(), 'no word took two photons'
    if nch > 1:
        assert ((hist != 0).sum(axis=1) >= 2).any(), 'no row with two touched channels'
        assert (timeless & (q > 0)).any(), 'no word with a history and a charge but no time'
    sizes = np.diff(bounds.astype(np.int64))
    touched = (hist != 0).any(axis=1)
    assert not touched[sizes == 0].any()
    assert sizes[0] == 0 and sizes[-1] == 0
    middle = [r for r in range(1, nrows - 1) if sizes[r] == 0 and touched[:r].any() and touched[r + 1:].any()]
    assert middle, 'no empty event between two that touched something'
    for origin in (0, int(bounds[0])):
        for edge in (64, 256):
            lo, hi = bounds[:-1].astype(np.int64) - origin, bounds[1:].astype(np.int64) - origin
            crossing = (sizes > 0) & (lo // edge != (hi - 1) // edge) & touched
            assert crossing.any(), 'no touched event across a multiple of %d from %d' % (edge, origin)
    assert (sizes > 256).any()
    runs = np.flatnonzero((sizes[:-2] == 1) & (sizes[1:-1] == 1) & (sizes[2:] == 1))
    assert len(runs) >= 2
    # the guard photons: outside every event; a window over them fires channels that no row has fired
    ph = rows[0]
    tables, unit = daq_tables(geo)
    for start, n in ((0, int(bounds[0])), (int(bounds[-1]), len(ph) - int(bounds[-1]))):
        fired = oracle_mod.run_daq(geo.packed, ph, tables, unit, seed=9, photon_id_base=DAQ_BASE, acquisition=BASE, weight=1.0, start_photon=start, nphotons=n)[2] != 0
        assert fired.any()
        if nch > 1:
            assert not hist[:, fired].any(), 'a channel of the guard photons is touched'


def test_many_event_inputs_touch_the_first_and_the_last_word(host_geos, expected):
    geo = host_geos['tiny']
    rows, bounds, state = expected('tiny', 'many')
    nrows = len(bounds) - 1
    hist = state[2].reshape(nrows, geo.nchannels)
    assert hist[0, 0] != 0 and hist[-1, -1] != 0, 'the gate let none of the three photons on the first (last) word through'
    touched = (hist != 0).sum(axis=1)
    assert (touched == 0).sum() > 100 and (touched >= 2).sum() > 10 and nrows * geo.nchannels > 2 ** 16 + 257
    assert (np.diff(bounds.astype(np.int64)) <= 3).all()


# ---- on the GPU ------------------------------------------------------------------------------------------------------------
@gpu_test
@pytest.mark.parametrize('which', ['tiny', 'stress'])
def test_acquire_events_is_the_oracle_row_by_row(gpu, geos, expected, which):
    """chroma_daq_acquire_events + chroma_daq_convert: the dense arrays are the stacked per-row oracle results; the words
    behind the last row keep what the test put there.  GPUEventDaq.acquire: every EventChannels[i] is the oracle's row i, and
    sparse(i) its touched channels.  On 'stress' the detector is one channel: the stride is 1, every event sits on one hot
    word and the rows are neighbouring words."""
    from chroma_amd import _lib
    from chroma_amd.gpu.tools import to_gpu
    geo = geos[which]
    rows, bounds, state = expected(which)
    nrows, nch = len(bounds) - 1, geo.nchannels
    words = nrows * nch
    daq = tables_of(gpu, geo)
    dev = upload(rows)
    arrays = device_state(gpu, words)
    call(gpu, 'chroma_daq_reset', 1e9, words, arrays[0].ptr, arrays[1].ptr, arrays[2].ptr)
    acquire_events(gpu, geo, daq, dev, bounds, arrays)
    assert_state(arrays, state, words, which)
    t, q = to_gpu(np.full(words, SENTINEL, dtype=np.uint32).view(np.float32)), to_gpu(np.full(words, SENTINEL, dtype=np.uint32).view(np.float32))
    call(gpu, 'chroma_daq_convert', words, daq.charge_unit, arrays[0].ptr, arrays[1].ptr, t.ptr, q.ptr)
    want_q = (state[1].astype(np.float32) * np.float32(daq.charge_unit)).astype(np.float32)
    assert np.array_equal(t.get().view(np.uint32), state[0]) and np.array_equal(q.get().view(np.uint32), want_q.view(np.uint32))

    channels = gpu.GPUEventDaq(geo.gg).acquire(dev, _lib.Rng(9, DAQ_BASE), bounds, acquisition=BASE, weight=WEIGHT)
    assert isinstance(channels, gpu.EventChannels) and len(channels) == nrows
    offsets, channel, tbits, qs, flags = expected_sparse(geo, state, nrows)
    for r in range(nrows):
        assert_channels(channels[r], row_channels(geo, state, r), '%s, event %d' % (which, r))
        got = channels.sparse(r)
        w = slice(offsets[r], offsets[r + 1])
        assert np.array_equal(got[0], channel[w]) and np.array_equal(got[1].view(np.uint32), tbits[w]), 'sparse(%d)' % r
        assert np.array_equal(got[2].view(np.uint32), qs[w].view(np.uint32)) and np.array_equal(got[3], flags[w]), 'sparse(%d)' % r
    assert_channels(channels[-1], row_channels(geo, state, nrows - 1), 'event -1')
    with pytest.raises(IndexError):
        channels[nrows]


@gpu_test
@pytest.mark.parametrize('which', ['tiny', 'stress'])
def test_one_row_is_gpudaq_on_the_same_window(gpu, oracle_mod, geos, which):
    from chroma_amd import _lib
    geo = geos[which]
    rows = daq_rows(geo)
    dev = upload(rows)
    rng = _lib.Rng(9, DAQ_BASE)
    daq = gpu.GPUDaq(geo.gg)
    daq.acquisition = BASE
    daq.begin_acquire()
    daq.acquire(dev, rng, weight=WEIGHT, start_photon=DAQ_FIRST, nphotons=DAQ_N)
    want = daq.end_acquire().get()
    assert want.hit.any()
    channels = gpu.GPUEventDaq(geo.gg).acquire(dev, rng, [DAQ_FIRST, DAQ_FIRST + DAQ_N], acquisition=BASE, weight=WEIGHT)
    assert len(channels) == 1
    assert_channels(channels[0], (want.t, want.q, want.flags, want.hit), which)
    state = oracle_rows(oracle_mod, geo, rows[0], np.array([DAQ_FIRST, DAQ_FIRST + DAQ_N]))
    assert_channels(channels[0], row_channels(geo, state, 0), which + ', the oracle')


@gpu_test
@pytest.mark.parametrize('which', ['tiny', 'stress'])
def test_two_acquires_onto_one_state_without_a_reset(gpu, geos, expected, which):
    """Acquisitions BASE and BASE + nrows onto one state: the oracle acquiring twice onto its state per row; the compaction of
    that state is its touched words."""
    geo = geos[which]
    rows, bounds, once = expected(which)
    _, _, state = expected(which, acquires=2)
    assert not np.array_equal(once[1], state[1])
    nrows = len(bounds) - 1
    words = nrows * geo.nchannels
    daq = tables_of(gpu, geo)
    dev = upload(rows)
    arrays = device_state(gpu, words)
    call(gpu, 'chroma_daq_reset', 1e9, words, arrays[0].ptr, arrays[1].ptr, arrays[2].ptr)
    acquire_events(gpu, geo, daq, dev, bounds, arrays, acquisition=BASE)
    acquire_events(gpu, geo, daq, dev, bounds, arrays, acquisition=BASE + nrows)
    assert_state(arrays, state, words, which)
    capacity = min(2 * DAQ_N, words)
    ntouched, got = compact(gpu, geo, arrays, nrows, capacity, daq.charge_unit)
    assert_sparse(got, ntouched, expected_sparse(geo, state, nrows), nrows, capacity, which)


@gpu_test
def test_acquire_events_with_a_wider_channel_stride(gpu, geos, expected):
    """channel_stride = nchannels + 5, called directly: row r lands in [r * stride, r * stride + nchannels); the gap words keep
    the reset pattern and the guard words behind the last row what the test put there.  The compaction reads the same layout."""
    geo = geos['tiny']
    stride = geo.nchannels + 5
    rows, bounds, state = expected('tiny', stride=stride)
    nrows = len(bounds) - 1
    words = nrows * stride
    gap = np.arange(words) % stride >= geo.nchannels
    assert (state[0][gap] == RESET_BITS).all() and (state[1][gap] == 0).all() and (state[2][gap] == 0).all() and (state[2] != 0).sum() > nrows
    daq = tables_of(gpu, geo)
    arrays = device_state(gpu, words)
    call(gpu, 'chroma_daq_reset', 1e9, words, arrays[0].ptr, arrays[1].ptr, arrays[2].ptr)
    acquire_events(gpu, geo, daq, upload(rows), bounds, arrays, stride=stride)
    assert_state(arrays, state, words, 'stride %d' % stride)
    capacity = min(DAQ_N, nrows * geo.nchannels)
    ntouched, got = compact(gpu, geo, arrays, nrows, capacity, daq.charge_unit, stride=stride)
    assert_sparse(got, ntouched, expected_sparse(geo, state, nrows, stride=stride), nrows, capacity, 'stride %d' % stride)


@gpu_test
def test_compaction_across_scan_tiles(gpu, geos, expected):
    """Some 1300 rows of zero to three photons, more than 2^16 + 257 words: offsets, channel, t, q and flags against
    np.nonzero(history) of the oracle's stacked state in row-major order -- rows with nothing touched among them, and the
    first and the last word of the state touched."""
    geo = geos['tiny']
    rows, bounds, state = expected('tiny', 'many')
    nrows = len(bounds) - 1
    words = nrows * geo.nchannels
    daq = tables_of(gpu, geo)
    arrays = device_state(gpu, words)
    call(gpu, 'chroma_daq_reset', 1e9, words, arrays[0].ptr, arrays[1].ptr, arrays[2].ptr)
    acquire_events(gpu, geo, daq, upload(rows), bounds, arrays)
    assert_state(arrays, state, words, 'many rows')
    capacity = min(int(bounds[-1]) - int(bounds[0]), words)
    ntouched, got = compact(gpu, geo, arrays, nrows, capacity, daq.charge_unit)
    want = expected_sparse(geo, state, nrows)
    assert want[1][0] == 0 and want[0][1] > 0 and want[1][-1] == geo.nchannels - 1 and want[0][-2] < want[0][-1]
    assert (np.diff(want[0].astype(np.int64)) == 0).sum() > 100
    assert_sparse(got, ntouched, want, nrows, capacity, 'many rows')


@gpu_test
def test_the_result_does_not_depend_on_the_chunking(gpu, geos, expected):
    """The same 1300 events with max_entries that gives 1, 7 and all rows per chunk: identical EventChannels, the oracle's."""
    from chroma_amd import _lib
    geo = geos['tiny']
    rows, bounds, state = expected('tiny', 'many')
    nrows = len(bounds) - 1
    dev = upload(rows)
    offsets, channel, tbits, qs, flags = expected_sparse(geo, state, nrows)
    for rows_per_chunk in (1, 7, nrows):
        daq = gpu.GPUEventDaq(geo.gg, max_entries=rows_per_chunk * geo.nchannels + (geo.nchannels - 1 if rows_per_chunk > 1 else 0))
        assert daq.rows_per_chunk == rows_per_chunk
        channels = daq.acquire(dev, _lib.Rng(9, DAQ_BASE), bounds, acquisition=BASE, weight=WEIGHT)
        assert len(channels) == nrows
        what = '%d rows per chunk' % rows_per_chunk
        got = [np.concatenate([channels.sparse(r)[k] for r in range(nrows)]) for k in range(4)]
        assert np.array_equal([len(channels.sparse(r)[0]) for r in range(nrows)], np.diff(offsets.astype(np.int64))), what
        assert np.array_equal(got[0], channel) and np.array_equal(got[1].view(np.uint32), tbits), what
        assert np.array_equal(got[2].view(np.uint32), qs.view(np.uint32)) and np.array_equal(got[3], flags), what
        for r in (0, 1, 6, 7, 8, nrows // 2, nrows - 1):
            assert_channels(channels[r], row_channels(geo, state, r), '%s, event %d' % (what, r))


@gpu_test
def test_bad_bounds_are_refused_before_anything_is_launched(gpu, geos):
    """Descending bounds, a last bound beyond the set, nrows = 0 and a stride below the number of channels: the
    invalid-argument error, and the accumulators keep the sentinel they were filled with."""
    geo = geos['tiny']
    rows = daq_rows(geo)
    n = len(rows[0])
    dev = upload(rows)
    daq = tables_of(gpu, geo)
    words = 4 * geo.nchannels
    arrays = device_state(gpu, words)
    cases = [('descending', dict(bounds=[257, 300, 299, 400, 500])),
             ('beyond the set', dict(bounds=[257, 300, 400, 500, n + 1])),
             ('no rows', dict(bounds=[257], nrows=0)),
             ('a narrow stride', dict(bounds=[257, 300, 400, 500, 600], stride=geo.nchannels - 1))]
    for what, kw in cases:
        assert acquire_events_rc(gpu, geo, daq, dev, arrays=arrays, **kw) == ERR_INVALID, what
    gpu.get_context().synchronize()
    for a in arrays:
        assert (a.get() == SENTINEL).all()
    acquire_events(gpu, geo, daq, dev, [257, 300, 400, 500, n], arrays)          # (the end of the set itself is a bound like another)


@gpu_test
def test_simulation_runs_the_daq_of_a_batch_as_one_acquisition(gpu, tiny_geometry, monkeypatch):
    """40 events of 1 to 500 bomb photons and an empty one in one batch through Simulation.simulate(run_daq=True), then a
    second simulate call: ev.channels is what a GPUDaq begin_acquire / acquire(start_photon, nphotons) / end_acquire per event
    gives on the same propagated photons with the acquisitions numbered 0, 1, 2, ... across the two calls -- and simulate()
    itself makes no GPUDaq.acquire call."""
    from conftest import bomb
    from chroma_amd import _lib
    from chroma_amd.gpu import tools
    from chroma_amd.sim import Simulation
    previous = tools._current
    rng = np.random.default_rng(5)
    sizes = [1, 500] + rng.integers(1, 501, 38).tolist()
    first = [bomb(n, seed=100 + k) for k, n in enumerate(sizes)]
    first.insert(17, event.Photons())
    second = [bomb(n, seed=200 + k) for k, n in enumerate((300, 1, 2, 450, 64))]
    calls = []
    acquire = gpu.GPUDaq.acquire
    monkeypatch.setattr(gpu.GPUDaq, 'acquire', lambda self, *a, **kw: (calls.append(1), acquire(self, *a, **kw))[1])
    try:
        sim = Simulation(tiny_geometry, seed=21)
        acquisition, nhit = 0, 0
        for batch in (first, second):
            base = sim.rng_states.next_photon_id
            events = list(sim.simulate(batch, run_daq=True, keep_photons_end=True, max_steps=100))
            assert len(events) == len(batch) and not calls, 'simulate() made %d GPUDaq.acquire calls' % len(calls)
            assert sim.gpu_daq.acquisition == acquisition + len(batch)
            with sim.context.bound():
                ends = event.Photons.join([ev.photons_end for ev in events])
                gp = gpu.GPUPhotons(ends)
                daq = gpu.GPUDaq(sim.gpu_geometry)
                daq.acquisition = acquisition
                lo = 0
                for k, ev in enumerate(events):
                    n = len(ev.photons_end)
                    assert n == len(batch[k])
                    daq.begin_acquire()
                    daq.acquire(gp, _lib.Rng(sim.seed, base), start_photon=lo, nphotons=n)
                    want = daq.end_acquire().get()
                    assert_channels(ev.channels, (want.t, want.q, want.flags, want.hit), 'event %d' % ev.id)
                    nhit += int(want.hit.sum())
                    lo += n
                acquisition = daq.acquisition
                del calls[:]
        assert nhit > 20
        del sim, gp, daq
    finally:
        tools._current = previous
