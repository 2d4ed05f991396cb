"""The photon-array, hit, DAQ and sort calls -- the "separate calls" other GPU tests take as the truth -- on NumPy.

chroma_photon_duplicate, chroma_count_photons / chroma_copy_photons (GPUPhotons.select), chroma_copy_photon_queue,
chroma_count_photon_hits / chroma_copy_photon_hits (get_flat_hits), chroma_channel_hits, the DAQ (GPUDaq), and the two
device sorts (sort_by_direction, chroma_hits_sort).  No propagation runs here: the photon arrays are written in NumPy with a
fixed seed -- flags, last hit triangles, times, weights and event indices as the case needs them -- and uploaded; the
expectation is plain NumPy (the DAQ: the oracle's run_daq / run_daq_many).  Every comparison is bit for bit, in all ten
arrays of a photon set (the nine of event.Photons and the draw counters).

Guard rows everywhere: the source arrays carry rows before ``first_photon`` and after ``first_photon + n`` that WOULD match
(flag set, triangle on a channel); destination arrays are longer than the expected count and pre-filled with a sentinel bit
pattern in every field, which the rows at and beyond the returned count must still hold; channel arrays carry guard words
past their end.  An off-by-one or an overrun shows as a wrong value, never as an access out of bounds.

Sizes: the edges of a wave (64), of a block (256) and of a copy block (COPY_ITEMS * 256 = 4096), a mid size with a window
from 0 and from 257, and for the two counting kernels 2^20 + 257 elements: their grid is capped at 4096 blocks of 256, so
only beyond 2^20 elements does their grid-stride loop turn.
"""
import ctypes

import numpy as np
import pytest

from chroma_amd import event
from chroma_amd.event import Photons
from conftest import make_stress_geometry
from test_gpu_parity import FIELDS, assert_bit_exact

gpu_test = pytest.mark.gpu          # (per test, not per module: the derivation of the direction codes is checked without a GPU)

SENTINEL = 0xA5A5A5A5               # as a float: -2.87e-16, an ordinary number (copies through float registers keep its bits)
SIZES = [1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8193]
WINDOWS = [(n, 3) for n in SIZES] + [(20000, 0), (20000, 257)]          # (n, first_photon)
TAIL = 70                           # guard rows behind a window
DETECT = event.SURFACE_DETECT
INF_BITS = 0x7f800000               # +inf: what GPUPhotons.channel_hits starts the earliest times from


@pytest.fixture(scope='module')
def gpu():
    from chroma_amd import gpu as g
    ctx = g.create_cuda_context(0)
    yield g
    ctx.pop()


class _Geo(object):
    """A detector on the device with what NumPy needs to restate the hit rule: the channel of every triangle."""

    def __init__(self, geometry, packed):
        self.geometry, self.packed = geometry, packed
        self.gg = None                                           # the GPUDetector, once a test with a GPU asks (geos)
        self.nchannels = geometry.num_channels()
        to_channel = np.asarray(geometry.solid_id_to_channel_index, dtype=np.int32)
        self.channel_of_triangle = to_channel[np.asarray(geometry.solid_id)]
        self.on = np.flatnonzero(self.channel_of_triangle >= 0)
        self.off = np.flatnonzero(self.channel_of_triangle < 0)
        assert len(self.on) and len(self.off)

    def triangles_of(self, channels):
        return np.flatnonzero(np.isin(self.channel_of_triangle, channels))


@pytest.fixture(scope='module')
def host_geos(tiny_geometry, tiny_packed):
    """'tiny': a few dozen channels, most solids without one; 'stress': the detector is ONE channel (the one-channel path of
    k_channel_hits and the hot word of the DAQ's atomics)."""
    from chroma_amd.gpu.geometry import pack_geometry
    stress = make_stress_geometry()
    out = {'tiny': _Geo(tiny_geometry, tiny_packed), 'stress': _Geo(stress, pack_geometry(stress))}
    assert out['tiny'].nchannels > 10 and out['stress'].nchannels == 1
    return out


@pytest.fixture(scope='module')
def geos(gpu, host_geos):
    for geo in host_geos.values():
        if geo.gg is None:
            geo.gg = gpu.GPUDetector(geo.geometry)
            assert geo.gg.nchannels == geo.nchannels
    return host_geos


# ---- photon sets on the host: (event.Photons, draw counters) ---------------------------------------------------------------
def make_photons(rng, n):
    """n photons of random bits in every field; pos.x is the row number, so every row is distinct and a comparison of two
    sets in a canonical order is a bijection.  Flags 0 and no last hit: the case sets them."""
    pos = rng.normal(0.0, 100.0, (n, 3)).astype(np.float32)
    pos[:, 0] = np.arange(n, dtype=np.float32) + np.float32(0.25)
    ph = Photons(pos, rng.normal(size=(n, 3)).astype(np.float32), rng.normal(size=(n, 3)).astype(np.float32),
                 rng.uniform(300.0, 700.0, n).astype(np.float32), t=rng.uniform(0.0, 100.0, n).astype(np.float32),
                 weights=rng.uniform(0.0, 1.0, n).astype(np.float32), evidx=rng.integers(0, 2 ** 32, n, dtype=np.uint32))
    return ph, rng.integers(0, 2 ** 32, n, dtype=np.uint32)


def sentinel(n):
    """n rows that hold the sentinel bit pattern in every field."""
    w = lambda *shape: np.full(shape, SENTINEL, dtype=np.uint32)
    f = lambda *shape: w(*shape).view(np.float32)
    ph = Photons(f(n, 3), f(n, 3), f(n, 3), f(n), t=f(n), last_hit_triangles=w(n).view(np.int32), flags=w(n), weights=f(n), evidx=w(n))
    return ph, w(n)


def take(rows, key):
    return rows[0][key], rows[1][key]


def put(rows, key, values):
    for name in FIELDS:
        getattr(rows[0], name)[key] = getattr(values[0], name)
    rows[1][key] = values[1]


def canonical_order(rows, extra=()):
    """The order of ``rows`` by their own content: a lexsort over the full record (and ``extra`` columns)."""
    ph, counters = rows
    keys = [counters, ph.evidx, ph.weights.view(np.uint32), ph.flags, ph.last_hit_triangles, ph.t.view(np.uint32), ph.wavelengths.view(np.uint32)]
    keys += [a.view(np.uint32)[:, k] for a in (ph.pol, ph.dir, ph.pos) for k in (2, 1, 0)]
    return np.lexsort(list(extra) + keys)


def upload(rows):
    from chroma_amd.gpu.photon import GPUPhotonsSlice
    from chroma_amd.gpu.tools import to_gpu, to_float3
    ph, counters = rows
    return GPUPhotonsSlice(pos=to_gpu(to_float3(ph.pos)), dir=to_gpu(to_float3(ph.dir)), pol=to_gpu(to_float3(ph.pol)),
                           wavelengths=to_gpu(ph.wavelengths), t=to_gpu(ph.t), last_hit_triangles=to_gpu(ph.last_hit_triangles),
                           flags=to_gpu(ph.flags), weights=to_gpu(ph.weights), evidx=to_gpu(ph.evidx), rng_counters=to_gpu(counters))


def fetch(dev):
    return dev.get(), dev.rng_counters.get()


def assert_same(got, want, what):
    """All ten arrays, bit for bit, row by row."""
    assert len(got[0]) == len(want[0]) == len(got[1]) == len(want[1]), '%s: %d rows, expected %d' % (what, len(got[0]), len(want[0]))
    assert_bit_exact(got[0], want[0], what)
    same = got[1] == want[1]
    assert same.all(), '%s: rng_counters differs for %d of %d photons (first at %s)' % (what, np.count_nonzero(~same), len(same), np.argwhere(~same)[0])


def assert_same_set(got, want, what, got_extra=(), want_extra=()):
    """The same rows in any order (the compactions go through an atomic); ``extra``: columns that travel with the rows."""
    assert len(got[0]) == len(want[0]), '%s: %d rows, expected %d' % (what, len(got[0]), len(want[0]))
    a, b = canonical_order(got, got_extra), canonical_order(want, want_extra)
    assert_same(take(got, a), take(want, b), what)
    for x, y in zip(got_extra, want_extra):
        assert np.array_equal(x[a], y[b]), '%s: a column beside the rows differs' % what


def call(g, name, *args):
    from chroma_amd import _lib
    ctx = g.get_context()
    _lib.check(getattr(ctx._lib, name)(ctx.handle, *args))


def structure(dev):
    from chroma_amd.gpu.photon import _structure
    return _structure(dev)


def windowed(rng, n, first):
    """first + n + TAIL photons; the window [first, first + n) and the mask of the guard rows around it."""
    total = first + n + TAIL
    rows = make_photons(rng, total)
    guard = np.ones(total, dtype=bool)
    guard[first:first + n] = False
    return rows, guard


def draw_triangles(rng, geo, n, on=None):
    """Last hit triangles from the four sets: on a channel, on no channel, -1, below -1 (no triangle for the kernels)."""
    on = geo.on if on is None else on
    kind = rng.choice(4, size=n, p=[0.55, 0.2, 0.15, 0.1])
    tri = np.where(kind == 0, rng.choice(on, size=n), rng.choice(geo.off, size=n))
    tri = np.where(kind == 2, -1, tri)
    tri = np.where(kind == 3, rng.choice([-2, -3, -1000, -2 ** 31], size=n), tri)
    return tri.astype(np.int32)


def draw_flags(rng, n, state, p=0.6):
    """Histories of assorted bits; a bit of ``state`` in a fraction p of them, none in the others."""
    other = np.array([event.NO_HIT, event.RAYLEIGH_SCATTER, event.REFLECT_DIFFUSE, event.SURFACE_TRANSMIT, event.BULK_REEMIT], dtype=np.uint32)
    other = other[(other & np.uint32(state)) == 0]
    flags = np.zeros(n, dtype=np.uint32)
    for bit in other:
        flags |= np.where(rng.random(n) < 0.4, bit, np.uint32(0)).astype(np.uint32)
    bits = np.array([1 << k for k in range(32) if state >> k & 1], dtype=np.uint32)
    flags |= np.where(rng.random(n) < p, rng.choice(bits, size=n), np.uint32(0)).astype(np.uint32)
    return flags


def expected_channels(geo, flags, triangles, state):
    """propagate.cu:157-171 in NumPy: ``history & state``, ``triangle > -1``, ``channel >= 0``; -1 where it is no hit."""
    channel = np.full(len(flags), -1, dtype=np.int64)
    ok = ((flags & np.uint32(state)) != 0) & (triangles > -1)
    channel[ok] = geo.channel_of_triangle[triangles[ok]]
    return channel


# ---- 1. count / copy / select ----------------------------------------------------------------------------------------------
@gpu_test
@pytest.mark.parametrize('n,first', WINDOWS)
def test_count_copy_select_over_a_window(gpu, n, first):
    """chroma_count_photons, chroma_copy_photons and GPUPhotons.select over [first, first + n): a single bit, a mask of which
    any bit matches, a mask nothing matches and a mask everything matches.  The guard rows have every bit set."""
    rng = np.random.default_rng(1000 * n + first)
    rows, guard = windowed(rng, n, first)
    ph = rows[0]
    every, never = 1 << 13, 1 << 20
    bits = np.array([1 << 2, 1 << 3, 1 << 4, 1 << 9], dtype=np.uint32)
    ph.flags[:] = np.uint32(every)
    for bit in bits:
        ph.flags[:] |= np.where(rng.random(len(ph)) < 0.4, bit, np.uint32(0)).astype(np.uint32)
    ph.flags[guard] = 0xFFFFFFFF
    src = upload(rows)
    s_src = structure(src)
    for mask, what in ((1 << 3, 'one bit'), ((1 << 2) | (1 << 9) | never, 'any of several bits'), (never, 'no match'), (every, 'every photon')):
        what = '%s, %d photons from %d' % (what, n, first)
        want = first + np.flatnonzero(ph.flags[first:first + n] & np.uint32(mask))
        count = ctypes.c_uint32(12345)
        call(gpu, 'chroma_count_photons', first, n, mask, src.flags.ptr, ctypes.byref(count))
        assert count.value == len(want), what
        room = len(ph) + 9                                       # (room for every row of the source, whatever a wrong kernel takes)
        dst = upload(sentinel(room))
        s_dst = structure(dst)
        ncopied = ctypes.c_uint32(12345)
        call(gpu, 'chroma_copy_photons', first, n, mask, ctypes.byref(s_src), ctypes.byref(s_dst), ctypes.byref(ncopied))
        assert ncopied.value == count.value, what
        got = fetch(dst)
        assert_same_set(take(got, slice(0, len(want))), take(rows, want), what)
        assert_same(take(got, slice(len(want), None)), sentinel(room - len(want)), what + ': rows behind the copied ones')
        sel = src.select(mask, start_photon=first, nphotons=n)
        assert len(sel) == len(want), what
        assert_same_set(fetch(sel), take(rows, want), what + ' (select)')
    assert len(fetch(src.select(never, start_photon=first, nphotons=n))[0]) == 0
    assert_same(fetch(src), rows, 'the source arrays')


@gpu_test
def test_the_counting_kernels_past_their_grid_cap(gpu, geos):
    """2^20 + 257 elements from element 5: k_count_photons and k_count_hits run 4096 blocks of 256 threads at the most, so the
    last 257 elements are counted by the second turn of the grid-stride loop.  Both turns see matches.  Only what the kernels
    read is allocated: the flags for chroma_count_photons; flags and last hit triangles for chroma_count_photon_hits, every
    other pointer of its struct on one small array."""
    from chroma_amd import _lib
    from chroma_amd.gpu.tools import to_gpu
    geo = geos['tiny']
    n, first = (1 << 20) + 257, 5
    total = first + n + TAIL
    rng = np.random.default_rng(20)
    flags = draw_flags(rng, total, DETECT, p=0.3)
    triangles = draw_triangles(rng, geo, total)
    guard = np.ones(total, dtype=bool)
    guard[first:first + n] = False
    flags[guard] = 0xFFFFFFFF
    triangles[guard] = geo.on[0]
    window = slice(first, first + n)
    match = (flags[window] & np.uint32(DETECT)) != 0
    hit = expected_channels(geo, flags[window], triangles[window], DETECT) >= 0
    for m in (match, hit):
        assert m[:1 << 20].any() and m[1 << 20:].any() and not m[1 << 20:].all()
    d_flags, d_triangles, d_small = to_gpu(flags), to_gpu(triangles), to_gpu(np.zeros(4, dtype=np.uint32))
    count = ctypes.c_uint32(12345)
    call(gpu, 'chroma_count_photons', first, n, DETECT, d_flags.ptr, ctypes.byref(count))
    assert count.value == np.count_nonzero(match)
    s = _lib.PhotonArrays()
    for name, _ in _lib.PhotonArrays._fields_:
        setattr(s, name, d_small.ptr)
    s.flags, s.last_hit_triangles, s.rng_counters = d_flags.ptr, d_triangles.ptr, None
    count = ctypes.c_uint32(12345)
    call(gpu, 'chroma_count_photon_hits', geo.gg.handle, first, n, DETECT, ctypes.byref(s), ctypes.byref(count))
    assert count.value == np.count_nonzero(hit)


# ---- 2. copy_queue ---------------------------------------------------------------------------------------------------------
@gpu_test
@pytest.mark.parametrize('n,start', [(n, 5) for n in SIZES] + [(20000, 257)])
def test_copy_queue_from_a_start(gpu, n, start):
    """chroma_copy_photon_queue with a queue that is a random permutation with repeats and start_photon != 0: row start + i of
    the destination is row queue[start + i] of the source, in order, in all fields; the rows below start and behind
    start + n keep their sentinel.  GPUPhotons.copy_queue returns those n rows."""
    from chroma_amd.gpu.tools import to_gpu
    rng = np.random.default_rng(2000 * n + start)
    nsrc = n // 2 + 40
    rows = make_photons(rng, nsrc)
    rows[0].flags[:] = draw_flags(rng, nsrc, DETECT)
    rows[0].last_hit_triangles[:] = rng.integers(-3, 1000, nsrc)
    total = start + n + TAIL
    queue = rng.integers(0, nsrc, total).astype(np.uint32)
    src, dst, d_queue = upload(rows), upload(sentinel(total)), to_gpu(queue)
    s_src, s_dst = structure(src), structure(dst)
    call(gpu, 'chroma_copy_photon_queue', start, n, d_queue.ptr, ctypes.byref(s_src), ctypes.byref(s_dst))
    want = sentinel(total)
    put(want, slice(start, start + n), take(rows, queue[start:start + n]))
    assert_same(fetch(dst), want, 'copy_queue of %d photons from entry %d' % (n, start))
    assert_same(fetch(src.copy_queue(d_queue, n, start_photon=start)), take(rows, queue[start:start + n]), 'GPUPhotons.copy_queue from entry %d' % start)
    assert_same(fetch(src.copy_queue(d_queue, n)), take(rows, queue[:n]), 'GPUPhotons.copy_queue from entry 0')
    assert_same(fetch(src), rows, 'the source arrays')


# ---- 3. duplicate ----------------------------------------------------------------------------------------------------------
@gpu_test
@pytest.mark.parametrize('copies', [1, 3])
@pytest.mark.parametrize('n,first', [(n, 3) for n in SIZES] + [(20000, 257)])
def test_photon_duplicate_with_a_window_and_a_stride(gpu, n, first, copies):
    """chroma_photon_duplicate(first, n, copies, stride) with first != 0 and stride > n: copy i of photon first + k is row
    first + k + i * stride, equal to its original in all ten arrays; the gaps between the strides, the rows before first and
    behind the last copy keep their sentinel."""
    rng = np.random.default_rng(3000 * n + copies)
    stride = n + 7
    total = first + stride * copies + n + TAIL
    original = make_photons(rng, n)
    original[0].flags[:] = draw_flags(rng, n, DETECT)
    original[0].last_hit_triangles[:] = rng.integers(-3, 1000, n)
    rows = sentinel(total)
    put(rows, slice(first, first + n), original)
    dev = upload(rows)
    s = structure(dev)
    call(gpu, 'chroma_photon_duplicate', first, n, ctypes.byref(s), copies, stride)
    for i in range(1, copies + 1):
        put(rows, slice(first + i * stride, first + i * stride + n), original)
    assert_same(fetch(dev), rows, '%d copies of %d photons from %d, stride %d' % (copies, n, first, stride))


@gpu_test
@pytest.mark.parametrize('n', [1, 257, 4097])
def test_ncopies_clones_every_field(gpu, n):
    """GPUPhotons(ncopies=3): every field of every copy is its original's, and the draw counters of all start at 0."""
    rng = np.random.default_rng(3500 + n)
    ph, _ = make_photons(rng, n)
    ph.flags[:] = draw_flags(rng, n, DETECT)
    ph.last_hit_triangles[:] = rng.integers(-3, 1000, n)
    gp = gpu.GPUPhotons(ph, ncopies=3)
    assert len(gp) == 3 * n
    got = fetch(gp)
    for k in range(3):
        assert_same(take(got, slice(k * n, (k + 1) * n)), (ph, np.zeros(n, dtype=np.uint32)), 'copy %d of %d photons' % (k, n))


# ---- 4. count / copy hits --------------------------------------------------------------------------------------------------
HIT_CASES = [('tiny', n, first, DETECT, 'mixed') for n, first in WINDOWS] + \
            [('stress', 65, 3, DETECT, 'mixed'), ('stress', 4097, 3, DETECT, 'mixed'), ('stress', 20000, 257, DETECT, 'mixed'),
             ('tiny', 4097, 3, event.SURFACE_ABSORB | event.BULK_ABSORB, 'mixed'), ('tiny', 4097, 3, DETECT, 'none'),
             ('tiny', 4097, 3, DETECT, 'all'), ('stress', 4097, 3, DETECT, 'all')]


def hit_rows(rng, geo, n, first, state, mode='mixed'):
    rows, guard = windowed(rng, n, first)
    ph = rows[0]
    ph.flags[:] = draw_flags(rng, len(ph), state)
    ph.last_hit_triangles[:] = draw_triangles(rng, geo, len(ph))
    if mode == 'none':               # the flag only where there is no channel, a channel only where there is no flag
        would = expected_channels(geo, ph.flags, ph.last_hit_triangles, state) >= 0
        ph.flags[would] &= ~np.uint32(state)
    elif mode == 'all':
        ph.flags[:] |= np.uint32(state & -state)
        ph.last_hit_triangles[:] = rng.choice(geo.on, size=len(ph))
    ph.flags[guard] |= np.uint32(state)
    ph.last_hit_triangles[guard] = rng.choice(geo.on, size=np.count_nonzero(guard))
    return rows


@gpu_test
@pytest.mark.parametrize('which,n,first,state,mode', HIT_CASES)
def test_count_and_copy_hits_over_a_window(gpu, geos, which, n, first, state, mode):
    """chroma_count_photon_hits, chroma_copy_photon_hits and get_flat_hits(device=True) over [first, first + n) against the
    rule ``history & state``, ``triangle > -1``, ``channel >= 0`` written in NumPy from solid_id and
    solid_id_to_channel_index: the count, the full records with their draw counters, the channels."""
    from chroma_amd.gpu.tools import to_gpu
    geo = geos[which]
    rng = np.random.default_rng(4000 * n + first + state)
    rows = hit_rows(rng, geo, n, first, state, mode)
    ph = rows[0]
    channel = expected_channels(geo, ph.flags, ph.last_hit_triangles, state)
    want = first + np.flatnonzero(channel[first:first + n] >= 0)
    what = '%s, %d photons from %d, state 0x%x, %s' % (which, n, first, state, mode)
    assert {'none': len(want) == 0, 'all': len(want) == n}.get(mode, True)
    assert (channel[:first] >= 0).all() and (channel[first + n:] >= 0).all(), 'guard rows that would not match'
    src = upload(rows)
    s_src = structure(src)
    count = ctypes.c_uint32(12345)
    call(gpu, 'chroma_count_photon_hits', geo.gg.handle, first, n, state, ctypes.byref(s_src), ctypes.byref(count))
    assert count.value == len(want), what
    room = len(ph) + 9                                           # (room for every row of the source, whatever a wrong kernel takes)
    dst = upload(sentinel(room))
    d_channels = to_gpu(np.full(room, SENTINEL, dtype=np.uint32).view(np.int32))
    s_dst = structure(dst)
    ncopied = ctypes.c_uint32(12345)
    call(gpu, 'chroma_copy_photon_hits', geo.gg.handle, first, n, state, ctypes.byref(s_src), ctypes.byref(s_dst), d_channels.ptr, ctypes.byref(ncopied))
    assert ncopied.value == len(want), what
    got, got_channels = fetch(dst), d_channels.get()
    k = len(want)
    assert_same_set(take(got, slice(0, k)), take(rows, want), what, (got_channels[:k].astype(np.int64),), (channel[want],))
    assert_same(take(got, slice(k, None)), sentinel(room - k), what + ': rows behind the hits')
    assert (got_channels[k:].view(np.uint32) == SENTINEL).all(), what + ': channels behind the hits'
    found, found_channels = src.get_flat_hits(geo.gg, target_flag=state, start_photon=first, nphotons=n, device=True)
    assert_same_set(fetch(found), take(rows, want), what + ' (get_flat_hits)', (found_channels.get().astype(np.int64),), (channel[want],))
    if k:
        flat = src.get_flat_hits(geo.gg, target_flag=state, start_photon=first, nphotons=n)
        assert np.array_equal(np.sort(flat.channel), np.sort(channel[want]).astype(np.uint32))
    assert_same(fetch(src), rows, 'the source arrays')


# ---- 5. per-channel counts and earliest times ------------------------------------------------------------------------------
GUARD_WORDS = 8


def channel_arrays(geo, counts=None, earliest=None):
    """Device (counts, earliest) of nchannels words and GUARD_WORDS sentinel words behind them."""
    from chroma_amd.gpu.tools import to_gpu
    c = np.full(geo.nchannels + GUARD_WORDS, SENTINEL, dtype=np.uint32)
    e = c.copy()
    c[:geo.nchannels] = 0 if counts is None else counts
    e[:geo.nchannels] = INF_BITS if earliest is None else earliest
    return to_gpu(c), to_gpu(e)


def expected_channel_hits(geo, ph, n, state, counts=None, earliest=None):
    """Counts and earliest-time bits after one more call over the first n photons: the count per channel added, the UNSIGNED
    minimum of the times' float bits taken (cuda/daq.cu:5-20: atomicMin on the bits)."""
    channel = expected_channels(geo, ph.flags[:n], ph.last_hit_triangles[:n], state)
    hit = channel >= 0
    counts = np.zeros(geo.nchannels, dtype=np.uint32) if counts is None else counts.copy()
    earliest = np.full(geo.nchannels, INF_BITS, dtype=np.uint32) if earliest is None else earliest.copy()
    counts += np.bincount(channel[hit], minlength=geo.nchannels).astype(np.uint32)
    np.minimum.at(earliest, channel[hit], ph.t[:n][hit].view(np.uint32))
    return counts, earliest


def run_channel_hits(g, geo, dev, n, state, d_counts, d_earliest):
    s = structure(dev)
    call(g, 'chroma_channel_hits', geo.gg.handle, n, state, ctypes.byref(s), d_counts.ptr, d_earliest.ptr if d_earliest is not None else None)
    c = d_counts.get()
    assert (c[geo.nchannels:] == SENTINEL).all(), 'guard words behind the counts'
    if d_earliest is None:
        return c[:geo.nchannels], None
    e = d_earliest.get()
    assert (e[geo.nchannels:] == SENTINEL).all(), 'guard words behind the earliest times'
    return c[:geo.nchannels], e[:geo.nchannels]


def channel_rows(rng, geo, n, state=DETECT):
    """n photons and TAIL rows behind them that would all count."""
    rows = make_photons(rng, n + TAIL)
    ph = rows[0]
    ph.flags[:] = draw_flags(rng, len(ph), state)
    ph.last_hit_triangles[:] = draw_triangles(rng, geo, len(ph))
    ph.flags[n:] |= np.uint32(state)
    ph.last_hit_triangles[n:] = rng.choice(geo.on, size=TAIL)
    ph.t[n:] = 0.0
    return rows


@gpu_test
@pytest.mark.parametrize('n', SIZES + [20000])
@pytest.mark.parametrize('which', ['tiny', 'stress'])
def test_channel_hits_and_a_second_call_onto_them(gpu, geos, which, n):
    """chroma_channel_hits on both geometries: counts and earliest-time bits are NumPy's; a second call with other photons onto
    the arrays the first left gives the sum of the counts and the minimum of the times (what the all-reduce relies on)."""
    geo = geos[which]
    rng = np.random.default_rng(5000 * n + len(which))
    d_counts, d_earliest = channel_arrays(geo)
    counts = earliest = None
    for k in range(2):
        rows = channel_rows(rng, geo, n)
        counts, earliest = expected_channel_hits(geo, rows[0], n, DETECT, counts, earliest)
        got_counts, got_earliest = run_channel_hits(gpu, geo, upload(rows), n, DETECT, d_counts, d_earliest)
        what = '%s, %d photons, call %d' % (which, n, k)
        assert np.array_equal(got_counts, counts), what
        assert np.array_equal(got_earliest, earliest), what
    assert n < 64 or counts.sum() > 0


def crafted_waves(rng, geo, last):
    """4 full waves and a last one of ``last`` lanes: (0) all 64 lanes on channel A; (1) 63 lanes on A and lane 17 on B (on
    the one-channel geometry: lane 17 is no hit); (2) a single hitter, in lane 63, the others every kind of no hit; (3) no
    hitter at all; (4, in the second block) ``last`` lanes, all on B."""
    n = 4 * 64 + last
    rows = make_photons(rng, n + TAIL)
    ph = rows[0]
    channels = np.unique(geo.channel_of_triangle[geo.on])
    a, b = channels[0], channels[-1]
    tri_a, tri_b = geo.triangles_of([a]), geo.triangles_of([b])
    ph.flags[:] = DETECT | event.REFLECT_DIFFUSE
    ph.last_hit_triangles[0:128] = rng.choice(tri_a, size=128)
    if a != b:
        ph.last_hit_triangles[64 + 17] = tri_b[0]
    else:
        ph.last_hit_triangles[64 + 17] = geo.off[0]
    miss = draw_triangles(rng, geo, 128, on=geo.off)             # off a channel, -1, below -1
    ph.last_hit_triangles[128:256] = miss
    ph.flags[128:256:2] = event.REFLECT_DIFFUSE                # ... and half of them without the flag
    ph.last_hit_triangles[128 + 63] = tri_a[-1]
    ph.flags[128 + 63] = DETECT
    ph.last_hit_triangles[256:] = rng.choice(tri_b, size=last + TAIL)
    return rows, n


@gpu_test
@pytest.mark.parametrize('last', [1, 63])
@pytest.mark.parametrize('which', ['tiny', 'stress'])
def test_channel_hits_on_crafted_waves(gpu, geos, which, last):
    """The two paths of k_channel_hits wave by wave: a wave whose hitters share a channel adds its popcount with one atomic,
    a wave with one dissenting lane adds lane by lane; a single hitter in the last lane; a last wave of 1 and of 63 lanes."""
    geo = geos[which]
    rows, n = crafted_waves(np.random.default_rng(5500 + last), geo, last)
    counts, earliest = expected_channel_hits(geo, rows[0], n, DETECT)
    assert counts.sum() == (64 + 64 + 1 + last if which == 'tiny' else 64 + 63 + 1 + last)
    d_counts, d_earliest = channel_arrays(geo)
    got_counts, got_earliest = run_channel_hits(gpu, geo, upload(rows), n, DETECT, d_counts, d_earliest)
    assert np.array_equal(got_counts, counts) and np.array_equal(got_earliest, earliest), (which, last)


@gpu_test
def test_channel_hits_without_earliest_times(gpu, geos):
    """d_earliest_time_bits == NULL: the same counts (asked once)."""
    geo = geos['tiny']
    n = 4097
    rows = channel_rows(np.random.default_rng(5600), geo, n)
    counts, _ = expected_channel_hits(geo, rows[0], n, DETECT)
    d_counts, _ = channel_arrays(geo)
    got_counts, _ = run_channel_hits(gpu, geo, upload(rows), n, DETECT, d_counts, None)
    assert np.array_equal(got_counts, counts) and counts.sum() > 1000


@gpu_test
@pytest.mark.parametrize('which', ['tiny', 'stress'])
def test_channel_hits_with_negative_times(gpu, geos, which):
    """Negative and -0.0 hit times.  The earliest time is the minimum over the times' raw float bits taken as UNSIGNED
    integers, as the reference's atomicMin on ``__float_as_int`` patterns of non-negative times intends (cuda/daq.cu:5-20; the
    kernel's comment says "non-negative times only").  A negative float has its sign bit set, so its pattern is ABOVE every
    non-negative one and above the +inf the arrays start from: a negative time never becomes a channel's earliest time, and a
    channel that saw only negative times keeps +inf while its count goes up.  That is the reference's own behaviour, pinned
    here as it is, not a defect of the kernel."""
    geo = geos[which]
    n = 8193
    rng = np.random.default_rng(5700)
    rows = channel_rows(rng, geo, n)
    ph = rows[0]
    ph.t[:n] = rng.uniform(-50.0, 50.0, n).astype(np.float32)
    ph.t[:n:7] = -0.0
    ph.t[3:n:11] = 0.0
    channels = np.unique(geo.channel_of_triangle[geo.on])
    only_negative = geo.channel_of_triangle[np.clip(ph.last_hit_triangles[:n], 0, None)] == channels[-1]
    if which == 'tiny':
        ph.t[:n][only_negative] = -np.abs(ph.t[:n][only_negative]) - np.float32(1.0)
    counts, earliest = expected_channel_hits(geo, ph, n, DETECT)
    assert (ph.t[:n] < 0).sum() > 1000 and (earliest < 0x80000000).all()         # no negative time is ever the earliest
    if which == 'tiny':
        assert counts[channels[-1]] > 0 and earliest[channels[-1]] == INF_BITS
    d_counts, d_earliest = channel_arrays(geo)
    got_counts, got_earliest = run_channel_hits(gpu, geo, upload(rows), n, DETECT, d_counts, d_earliest)
    assert np.array_equal(got_counts, counts) and np.array_equal(got_earliest, earliest)


# ---- 6. DAQ ----------------------------------------------------------------------------------------------------------------
DAQ_N, DAQ_FIRST = 3000, 257
DAQ_BASE = 2 ** 32 + 12345


def daq_rows(geo, seed=60):
    """DAQ_FIRST + DAQ_N + TAIL photons for the window [DAQ_FIRST, DAQ_FIRST + DAQ_N): weights in [0, 1], times around 0 (so
    some smeared times are negative).  With more than one channel: the last three channels get no photon of the window (they
    stay unfired; the guard rows sit on them with weight 1 and would fire them), and every photon on the first channel is 30
    to 40 ns early, so that channel sees negative times only."""
    rng = np.random.default_rng(seed)
    rows, guard = windowed(rng, DAQ_N, DAQ_FIRST)
    ph = rows[0]
    channels = np.unique(geo.channel_of_triangle[geo.on])
    dark = channels[-3:] if len(channels) > 1 else channels
    lit = channels[:-3] if len(channels) > 1 else channels
    ph.flags[:] = draw_flags(rng, len(ph), DETECT, p=0.8)
    ph.last_hit_triangles[:] = draw_triangles(rng, geo, len(ph), on=geo.triangles_of(lit))
    ph.t[:] = rng.uniform(-3.0, 3.0, len(ph)).astype(np.float32)
    if len(channels) > 1:
        early = geo.channel_of_triangle[np.clip(ph.last_hit_triangles, 0, None)] == channels[0]
        ph.t[early] = rng.uniform(-40.0, -30.0, np.count_nonzero(early)).astype(np.float32)
    ph.flags[guard] |= np.uint32(DETECT)
    ph.last_hit_triangles[guard] = rng.choice(geo.triangles_of(dark), size=np.count_nonzero(guard))
    ph.weights[guard] = 1.0
    return rows


def daq_tables(geo, daq=None):
    """(the four CDF tables, the charge unit) of a detector as GPUDaq makes them; with ``daq``: checked to be that DAQ's."""
    from chroma_amd.gpu.daq import _padded_cdf
    tables = _padded_cdf(*geo.geometry.time_cdf) + _padded_cdf(*geo.geometry.charge_cdf)
    unit = float(np.float32(geo.geometry.charge_cdf[0][-1] / 2 ** 16))
    if daq is not None:
        assert unit == daq.charge_unit and all(np.array_equal(a, b) for a, b in zip(tables, daq._tables_host))
    return tables, unit


def oracle_daq(oracle_mod, geo, ph, ndaq, state, **kw):
    """One acquire of the oracle onto ``state``; returns copies of (t, q, flags, hit) as GPUChannels.get() gives them."""
    tables, unit = daq_tables(geo)
    if ndaq == 1:
        out = oracle_mod.run_daq(geo.packed, ph, tables, unit, state=state, **kw)
    else:
        out = oracle_mod.run_daq_many(geo.packed, ph, tables, unit, ndaq=ndaq, state=state, **kw)
    return [np.array(a, copy=True) for a in out]


def assert_channels(got, want, what):
    t, q, hist, hit = want
    assert np.array_equal(got.t.view(np.uint32), t.view(np.uint32)), what + ': t'
    assert np.array_equal(got.q.view(np.uint32), q.view(np.uint32)), what + ': q'
    assert np.array_equal(got.flags, hist), what + ': flags'
    assert np.array_equal(got.hit, hit), what + ': hit'


DAQ_CASES = [('tiny', 1), ('tiny', 3), ('tiny', 64), ('tiny', 65), ('stress', 1), ('stress', 3)]
DAQ_WINDOW = dict(start_photon=DAQ_FIRST, nphotons=DAQ_N)


def daq_input_conditions(oracle_mod, geo, ph, ndaq, weight=0.7):
    """What the inputs must exercise, decided from the oracle's output alone, on the CPU.  Returns the figures."""
    kw = dict(seed=9, photon_id_base=DAQ_BASE, **DAQ_WINDOW)
    gated = oracle_daq(oracle_mod, geo, ph, ndaq, None, weight=weight, **kw)
    open_ = oracle_daq(oracle_mod, geo, ph, ndaq, None, weight=1.0, **kw)
    t, q, hist, hit = gated
    one_photon_most = np.float32(daq_tables(geo)[0][2][-1]) * np.float32(1.01)      # the largest charge ONE photon can add
    figures = dict(fired=int((hist != 0).sum()), fired_at_weight_1=int((open_[2] != 0).sum()), words=len(hist),
                   charge_differs=int((q != open_[1]).sum()), channels_with_two_or_more=int((q > one_photon_most).sum()),
                   # accepted photons (a history, a charge) whose times never became the earliest: the unsigned minimum over
                   # the float bits ranks every negative time above the reset value, so all their times were negative
                   fired_with_negative_times_only=int(((hist != 0) & ~hit).sum()), unfired=int((hist == 0).sum()))
    assert not (np.array_equal(hist != 0, open_[2] != 0) and np.array_equal(q, open_[1])), 'the weight gate rejected nothing'
    assert figures['channels_with_two_or_more'] >= 1
    if geo.nchannels > 1:
        assert figures['fired_with_negative_times_only'] >= 1 and figures['unfired'] >= 1
    return figures


@pytest.mark.parametrize('which,ndaq', DAQ_CASES)
def test_daq_inputs_exercise_the_gate_shared_channels_negative_times_and_dark_channels(oracle_mod, host_geos, which, ndaq):
    """Without a GPU: the DAQ inputs of the test below do what they are there for.  From the oracle's output alone: under the
    global weight 0.7 the fired channels or their charges are not those of weight 1 (the gate rejected something); a
    channel holds more charge than one photon can add (two or more accepted photons on one word); and, where there is more
    than one channel, a channel has a history and a charge but no time (every accepted time on it was negative: the unsigned
    minimum ranks those above the reset value) and a channel stays unfired."""
    geo = host_geos[which]
    figures = daq_input_conditions(oracle_mod, geo, daq_rows(geo)[0], ndaq)
    assert figures['fired'] < figures['words'] or geo.nchannels == 1


@gpu_test
@pytest.mark.parametrize('which,ndaq', DAQ_CASES)
def test_daq_weight_gate_window_and_two_acquires(gpu, oracle_mod, geos, which, ndaq):
    """GPUDaq against the oracle's run_daq / run_daq_many, bit for bit in t, q, flags and hit: per-photon weights in [0, 1]
    under a global weight of 0.7, a window of the photons, a photon id base beyond 2^32, and two acquires (acquisitions 0
    and 1) between one begin_acquire / end_acquire -- compared after the first and after the second.  With ndaq = 3, 64 and
    65 a photon's copies straddle a block of k_run_daq_many (256 is no multiple of 3 or 65)."""
    from chroma_amd import _lib
    geo = geos[which]
    rows = daq_rows(geo)
    ph = rows[0]
    window = DAQ_WINDOW
    daq = gpu.GPUDaq(geo.gg, ndaq=ndaq)
    daq_tables(geo, daq)
    daq_input_conditions(oracle_mod, geo, ph, ndaq)
    dev = upload(rows)
    rng = _lib.Rng(9, DAQ_BASE)
    state = oracle_mod.daq_state(geo.nchannels * ndaq)
    daq.begin_acquire()
    for acquisition in range(2):
        daq.acquire(dev, rng, weight=0.7, **window)
        want = oracle_daq(oracle_mod, geo, ph, ndaq, state, seed=9, photon_id_base=DAQ_BASE, acquisition=acquisition, weight=0.7, **window)
        assert_channels(daq.end_acquire().get(), want, '%s, ndaq %d, after acquire %d' % (which, ndaq, acquisition))
        if acquisition == 0:
            first = want
    assert not np.array_equal(first[1], want[1])                 # the second acquire did add to the first


@gpu_test
@pytest.mark.parametrize('ndaq', [1, 3])
def test_daq_global_weight_zero_fires_nothing(gpu, oracle_mod, geos, ndaq):
    from chroma_amd import _lib
    geo = geos['tiny']
    rows = daq_rows(geo)
    daq = gpu.GPUDaq(geo.gg, ndaq=ndaq)
    daq.begin_acquire()
    daq.acquire(upload(rows), _lib.Rng(9, DAQ_BASE), weight=0.0, start_photon=DAQ_FIRST, nphotons=DAQ_N)
    want = oracle_daq(oracle_mod, geo, rows[0], ndaq, None, seed=9, photon_id_base=DAQ_BASE, weight=0.0, start_photon=DAQ_FIRST, nphotons=DAQ_N)
    assert not want[3].any() and (want[2] == 0).all() and (want[1] == 0).all()
    assert_channels(daq.end_acquire().get(), want, 'weight 0, ndaq %d' % ndaq)


@gpu_test
def test_daq_acquire_many_with_a_wider_channel_stride(gpu, oracle_mod, geos):
    """chroma_daq_acquire_many called directly with channel_stride = nchannels + 5: copy i lands in [i * stride, i * stride +
    nchannels); the gap words and the guard words behind the last copy keep what chroma_daq_reset (the gaps) and the test
    (the guards) put there."""
    from chroma_amd import _lib
    from chroma_amd.gpu.tools import to_gpu
    geo = geos['tiny']
    ndaq, stride = 3, geo.nchannels + 5
    rows = daq_rows(geo)
    daq = gpu.GPUDaq(geo.gg, ndaq=ndaq)                          # (for its tables)
    words = ndaq * stride
    arrays = [to_gpu(np.full(words + GUARD_WORDS, SENTINEL, dtype=np.uint32)) for _ in range(3)]
    call(gpu, 'chroma_daq_reset', 1e9, words, arrays[0].ptr, arrays[1].ptr, arrays[2].ptr)
    dev = upload(rows)
    s = structure(dev)
    call(gpu, 'chroma_daq_acquire_many', geo.gg.handle, ctypes.byref(daq.tables), DAQ_FIRST, DAQ_N, DETECT, ctypes.byref(s), _lib.Rng(9, DAQ_BASE),
         0, 0.7, ndaq, stride, arrays[0].ptr, arrays[1].ptr, arrays[2].ptr)
    state = oracle_mod.daq_state(words)
    oracle_mod.run_daq_many(geo.packed, rows[0], daq._tables_host, daq.charge_unit, seed=9, ndaq=ndaq, photon_id_base=DAQ_BASE, weight=0.7,
                            start_photon=DAQ_FIRST, nphotons=DAQ_N, state=state, channel_stride=stride)
    gap = np.arange(words) % stride >= geo.nchannels
    assert (state[0][gap] == np.float32(1e9).view(np.uint32)).all() and (state[1][gap] == 0).all() and (state[2][gap] == 0).all()
    assert (state[2] != 0).sum() > ndaq
    for got, want, name in zip(arrays, state, ('time bits', 'charge counts', 'histories')):
        got = got.get()
        assert np.array_equal(got[:words], want), name
        assert (got[words:] == SENTINEL).all(), 'guard words behind the %s' % name


@gpu_test
def test_daq_from_a_slice_of_copies(gpu, oracle_mod, geos):
    """Acquiring from an iterate_copies() slice: the oracle's result with the parent's id base plus the slice's offset."""
    geo = geos['tiny']
    rows = daq_rows(geo, seed=61)
    ph = rows[0]
    n = len(ph)
    rng_states = gpu.get_rng_states(64, seed=77)
    rng_states.reserve(1000)                                     # the parent's block of ids does not start at 0
    gp = gpu.GPUPhotons(ph, ncopies=2)
    view = list(gp.iterate_copies())[1]
    daq = gpu.GPUDaq(geo.gg)
    daq.begin_acquire()
    daq.acquire(view, rng_states, weight=0.7)
    want = oracle_daq(oracle_mod, geo, ph, 1, None, seed=77, photon_id_base=1000 + n, weight=0.7)
    other = oracle_daq(oracle_mod, geo, ph, 1, None, seed=77, photon_id_base=1000, weight=0.7)
    assert not np.array_equal(want[0], other[0])
    assert_channels(daq.end_acquire().get(), want, 'second copy of two')


# ---- 7. sort_by_direction --------------------------------------------------------------------------------------------------
def direction_codes(oracle_mod, direction):
    """k_direction_codes (csrc/bvh_device.hip) restated: the contract's acos and atan2 from the oracle, every other operation
    in NumPy float32 in the kernel's order (the library is built with -ffp-contract=off, so each is rounded once, as here).
    Returns (codes, theta, phi)."""
    d = np.ascontiguousarray(direction, dtype=np.float32)
    one, pi, maxint = np.float32(1.0), np.float32(3.141592653589793), np.float32(65535.0)
    z = np.maximum(-one, np.minimum(one, d[:, 2]))
    theta = (oracle_mod.math_fn('acos', z) / pi * maxint)
    phi = ((oracle_mod.math_fn('atan2', d[:, 1], d[:, 0]) / pi / np.float32(2.0) + np.float32(0.5)) * maxint)
    assert theta.dtype == np.float32 and phi.dtype == np.float32
    theta, phi = theta.astype(np.uint32), phi.astype(np.uint32)
    codes = np.zeros(len(d), dtype=np.uint32)
    for b in range(16):
        bit = np.uint32(1 << b)
        codes |= ((theta & bit) << np.uint32(b)) | ((phi & bit) << np.uint32(b + 1))
    return codes, theta, phi


def direction_rows(rng, n):
    """n photons with directions on the sphere; where there is room: the poles, the x axis, the two ends of phi at
    (-1, +-0.0, 0), and runs of exact duplicates (a stable sort keeps their input order)."""
    rows = make_photons(rng, n)
    d = rows[0].dir
    d /= np.linalg.norm(d, axis=1)[:, None]
    special = np.array([[0, 0, 1], [0, 0, -1], [1, 0, 0], [-1, 0.0, 0], [-1, -0.0, 0], [0, 1, 0], [0, -1, 0]], dtype=np.float32)
    if n >= 100:
        d[10:10 + len(special)] = special
        d[50:50 + len(special)] = special[::-1]
        k = n // 5
        d[n - k:] = d[rng.integers(0, n - k, k)]                 # exact duplicates of earlier rows, in a random order
        assert np.signbit(d[10 + 4, 1]) and not np.signbit(d[10 + 3, 1])
    return rows


@gpu_test
@pytest.mark.parametrize('n', [0, 1, 2, 257, 8193, 200000])
def test_sort_by_direction_is_the_stable_argsort_of_the_contract_codes(gpu, oracle_mod, n):
    """After sort_by_direction EVERY row of all ten arrays is photons[np.argsort(codes, kind='stable')], the codes derived on
    the CPU from the contract's arc functions: no excluded fraction."""
    rows = direction_rows(np.random.default_rng(7000 + n), n)
    codes, _, _ = direction_codes(oracle_mod, rows[0].dir)
    order = np.argsort(codes, kind='stable')
    if n >= 257:
        assert len(np.unique(codes)) < n and (np.diff(order) < 0).any()
    dev = upload(rows)
    dev.sort_by_direction()
    assert_same(fetch(dev), take(rows, order), 'sort_by_direction of %d photons' % n)


def test_derived_direction_codes_are_argsort_direction_codes(oracle_mod):
    """Without a GPU: the codes test_sort_by_direction... derives are tools.argsort_direction's (chroma/tools.py:175-193), up to
    the last bits of the arc functions.  NumPy computes the angles with its own arccos / arctan2; the contract's differ from
    them by an ulp or two, which changes a truncated 16-bit angle only when the value sits that close to an integer.  So:
    wherever the two differ, they differ by ONE unit in theta or in phi, and the exact value lies within 4 ulp of a float32
    below 65536 (4 * 2^-8) of the integer between the two; the fraction of such rows is bounded by the chance of a value that
    close to an integer, 2 angles * 2 * 4 * 2^-8.  Measured on 2e6 directions: 413 thetas and 350 phis differ (3.8e-4 of the
    rows) against NumPy on float32 input, 3138 and 2915 (3.0e-3) against NumPy on float64 input -- more than the "few per
    million" the order of the sorted rows differs by, which is what the earlier GPU test saw."""
    from chroma_amd.tools import argsort_direction
    rng = np.random.default_rng(70)
    n = 1000000
    d = rng.normal(size=(n, 3))
    d = (d / np.linalg.norm(d, axis=1)[:, None]).astype(np.float32)
    codes, theta, phi = direction_codes(oracle_mod, d)
    maxint = 2 ** 16 - 1
    for given in (d, d.astype(np.float64)):
        np_theta_exact = np.arccos(np.clip(given[:, 2], -1, 1)) / np.pi * maxint
        np_phi_exact = (np.arctan2(given[:, 1], given[:, 0]) / np.pi / 2.0 + 0.5) * maxint
        np_theta, np_phi = np_theta_exact.astype(np.uint32), np_phi_exact.astype(np.uint32)
        np_codes = np.zeros(n, dtype=np.uint32)
        for i in range(16):
            bit = np.uint32(1 << i)
            np_codes |= ((np_theta & bit) << np.uint32(i)) | ((np_phi & bit) << np.uint32(i + 1))
        assert np.array_equal(np.argsort(np_codes, kind='stable'), argsort_direction(given))       # (they ARE the tool's codes)
        differing = 0
        for mine, theirs, exact in ((theta, np_theta, np_theta_exact), (phi, np_phi, np_phi_exact)):
            diff = mine.astype(np.int64) - theirs.astype(np.int64)
            rows = np.flatnonzero(diff)
            differing += len(rows)
            assert (np.abs(diff[rows]) == 1).all()
            between = np.maximum(mine[rows], theirs[rows]).astype(np.float64)
            assert (np.abs(exact[rows].astype(np.float64) - between) <= 4 * 2.0 ** -8).all()
        assert np.array_equal(codes != np_codes, (theta != np_theta) | (phi != np_phi))
        assert 0 < differing <= n * 2 * 2 * 4 * 2.0 ** -8


# ---- 8. chroma_hits_sort ---------------------------------------------------------------------------------------------------
@gpu_test
@pytest.mark.parametrize('with_counters', [True, False])
@pytest.mark.parametrize('n', [2, 257, 8193])
def test_hits_sort_is_the_stable_sort_by_event_and_channel(gpu, n, with_counters):
    """chroma_hits_sort on synthetic hits: event indices that include 0 and 2^32 - 1, channels with repeats.  The sort is
    stable, so the result is hits[np.lexsort((channel, evidx))] row by row, in every field and in the channel array; the rows
    behind the n hits keep their sentinel.  With rng_counters null the counters are left alone."""
    from chroma_amd.gpu.tools import to_gpu
    rng = np.random.default_rng(8000 + n)
    rows = make_photons(rng, n)
    rows[0].evidx[:] = rng.choice(np.array([0, 1, 7, 2 ** 31, 2 ** 32 - 1], dtype=np.uint32), size=n)
    rows[0].evidx[:2] = [2 ** 32 - 1, 0]
    rows[0].flags[:] = draw_flags(rng, n, DETECT)
    rows[0].last_hit_triangles[:] = rng.integers(0, 1000, n)
    channel = rng.integers(0, 6, n).astype(np.int32)
    channel[:2] = [3, 3]
    order = np.lexsort((channel, rows[0].evidx))
    assert n < 257 or (np.diff(order) < 0).any()
    padded = sentinel(n + TAIL)
    put(padded, slice(0, n), rows)
    dev = upload(padded)
    d_channel = to_gpu(np.r_[channel, np.full(TAIL, SENTINEL, dtype=np.uint32).view(np.int32)])
    s = structure(dev)
    if not with_counters:
        s.rng_counters = None
    call(gpu, 'chroma_hits_sort', ctypes.byref(s), d_channel.ptr, n)
    want = sentinel(n + TAIL)
    put(want, slice(0, n), take(rows, order))
    if not with_counters:
        want[1][:n] = rows[1]
    assert_same(fetch(dev), want, 'hits_sort of %d hits' % n)
    got_channel = d_channel.get()
    assert np.array_equal(got_channel[:n], channel[order]) and (got_channel[n:].view(np.uint32) == SENTINEL).all()
