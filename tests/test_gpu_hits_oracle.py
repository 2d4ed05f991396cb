"""chroma_propagate_hits -- the call bench.py times and Simulation makes -- against the CPU oracle.

tests/test_gpu_hits.py compares the fused call with the engine's own separate calls; every oracle comparison elsewhere goes through
GPUPhotons.propagate, which has no hits request.  Here the EXPECTED result of a fused call comes from the oracle alone
(expected_from_oracle: the oracle's end state and draw counters, then count/copy_photon_hits of propagate.cu:147-214 restated in
NumPy), and the call is made at the batch sizes where its path changes: the edges of a wave (64), of a k_finalize_hits block
(COPY_ITEMS * 256 = 4096) and of the tail policy (PROP_BLOCK * 16 * 8 = 8192).  What only the fused call has is under test: the
64-byte final records with their epoch, k_mark_tail, k_finalize_hits beside k_tail_coop, and the tail kernel's own hit writer.

Everything is bit-exact: there is no tolerance.  The numeric floors (hits > 50, alive > 100, launches) are properties of the
INPUTS, checked with the oracle alone; they keep a case from passing vacuously.
"""
import ctypes

import numpy as np
import pytest

from chroma_amd import event
from chroma_amd.event import Photons
from conftest import bomb, make_stress_geometry
from test_gpu_hits import canonical, fetch
from test_gpu_parity import assert_bit_exact, _edge_photons

gpu_test = pytest.mark.gpu          # (per test: test_derivation_of_the_expected_hits runs without a GPU)

NO_HIT_TIME = 0x7f800000            # +inf as bits: a channel nobody hit
FEW = 8192                          # the reference's "few photons left" (chroma/gpu/photon.py:227): the tail launch below it


# ---- the expected side: plain NumPy on the oracle's output ---------------------------------------------------------------------
class Expected(object):
    """What a fused call must return: photon arrays, draw counters, launches, and the hits derived from them."""

    def __init__(self, end, counters, launches, index, hits, hit_counters, counts, earliest):
        self.end, self.counters, self.launches = end, counters, launches
        self.index = index                              # ids of the photons that are hits
        self.hits, self.hit_counters = hits, hit_counters
        self.counts, self.earliest = counts, earliest
        self.nhits = len(index)


def derive_hits(geometry, end, counters, target_flag=event.SURFACE_DETECT):
    """count/copy_photon_hits (propagate.cu:147-214) and the per-channel arrays, from an end state: a hit is a photon with
    ``target_flag`` set, a last hit triangle, and a channel on that triangle's solid.  Returns (index, hits with channel, their
    draw counters, counts[nchannels], earliest[nchannels] as uint32 time bits)."""
    nchannels = geometry.num_channels()
    flagged = (end.flags & np.uint32(target_flag)) != 0
    tri = end.last_hit_triangles
    chan = np.full(len(end), -1, dtype=np.int64)
    ok = flagged & (tri > -1)
    chan[ok] = np.asarray(geometry.solid_id_to_channel_index)[np.asarray(geometry.solid_id)[tri[ok]]]
    index = np.flatnonzero(chan >= 0)
    hits = end[index]
    hits.channel = chan[index].astype(np.uint32)
    counts = np.bincount(chan[index], minlength=nchannels).astype(np.uint32)
    earliest = np.full(nchannels, NO_HIT_TIME, dtype=np.uint32)
    np.minimum.at(earliest, chan[index], end.t[index].view(np.uint32))
    return index, hits, np.asarray(counters, dtype=np.uint32)[index], counts, earliest


def expected_from_oracle(oracle_mod, geometry, packed, photons, seed, id_base=0, max_steps=100, use_weights=False, scatter_first=0,
                         rng_counters=None):
    end, counters, ostats = oracle_mod.propagate(packed, photons, seed, id_base, max_steps, use_weights, scatter_first, rng_counters,
                                                 nthreads=8)
    return Expected(end, counters, ostats['launches'], *derive_hits(geometry, end, counters))


# ---- the engine side -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def gpu():
    from chroma_amd import gpu as g
    ctx = g.create_cuda_context(0)
    yield g
    ctx.pop()


@pytest.fixture(scope='module')
def tiny(gpu, tiny_geometry, tiny_packed):
    return tiny_geometry, tiny_packed, gpu.GPUDetector(tiny_geometry)


@pytest.fixture(scope='module')
def stress(gpu):
    from chroma_amd.gpu.geometry import pack_geometry
    geometry = make_stress_geometry()
    return geometry, pack_geometry(geometry), gpu.GPUDetector(geometry)


def channel_arrays(g, gg):
    from chroma_amd.gpu.tools import zeros, GPUArray
    ctx = g.get_context()
    return zeros(gg.nchannels, np.uint32, ctx), GPUArray(gg.nchannels, np.uint32, ctx).fill(np.uint32(NO_HIT_TIME))


def assert_hits(got_hits, got_counters, want, what):
    assert len(got_hits) == want.nhits, '%s: %d flat hits, %d derived' % (what, len(got_hits), want.nhits)
    got_hits, got_counters = canonical(got_hits, got_counters)
    want_hits, want_counters = canonical(want.hits, want.hit_counters)
    assert_bit_exact(got_hits, want_hits, what + ', flat hits')
    assert np.array_equal(got_hits.channel, want_hits.channel), what + ': channels of the flat hits'
    different = np.flatnonzero(got_counters != want_counters)
    assert len(different) == 0, '%s: draw counters of %d of %d flat hits differ (first: got %d, want %d)' % (
        what, len(different), len(want_counters), got_counters[different[0]], want_counters[different[0]])


def assert_photons(gp, want, what):
    assert_bit_exact(gp.get(), want.end, what + ', photon arrays')
    assert np.array_equal(gp.rng_counters.get(), want.counters), what + ': draw counters of the photons'


def fused(g, oracle_mod, where, photons, seed=7, id_base=0, max_steps=100, ncopies=1, capacity=None, gp=None, want=None,
          counters_in=None, oracle_input=None, what='', **kw):
    """One GPUPhotons.propagate_hits call on ``photons`` (or on the device photons ``gp``, continued) checked against the oracle
    in every output.  ``kw``: use_weights, scatter_first for both sides; exact for the engine.  Returns (Expected, stats)."""
    from chroma_amd import _lib
    geometry, packed, gg = where
    if want is None:
        okw = {k: v for k, v in kw.items() if k != 'exact'}
        if oracle_input is None:
            oracle_input = photons if ncopies == 1 else Photons.join([photons] * ncopies)     # (clone c of photon i: id c * n + i)
        want = expected_from_oracle(oracle_mod, geometry, packed, oracle_input, seed, id_base, max_steps, rng_counters=counters_in, **okw)
    if gp is None:
        gp = g.GPUPhotons(photons, ncopies=ncopies)
    counts, earliest = channel_arrays(g, gg)
    stats = {}
    found = gp.propagate_hits(gg, _lib.Rng(seed, id_base), max_steps=max_steps, capacity=capacity, channel_arrays=(counts, earliest),
                              stats=stats, device=True, **kw)
    what = what or '%d photons, %d steps' % (len(gp), max_steps)
    assert_photons(gp, want, what)
    assert stats['nhits'] == want.nhits, '%s: nhits %d, derived %d' % (what, stats['nhits'], want.nhits)
    assert_hits(*fetch(*found), want, what)
    assert np.array_equal(counts.get(), want.counts), what + ': per-channel counts'
    assert np.array_equal(earliest.get(), want.earliest), what + ': per-channel earliest times'
    assert stats['launches'] == want.launches, '%s: %d launches, the oracle %d' % (what, stats['launches'], want.launches)
    return want, stats


def alive(end):
    return int(np.count_nonzero((end.flags & event.TERMINAL_MASK) == 0))


def preflagged(geometry, n=20000, seed=8):
    """The input of test_gpu_hits.py's "terminal before the call": every seventh photon detected before the call on a chosen
    triangle -- every third of those on a triangle of a solid WITHOUT a channel."""
    ph = bomb(n, seed)
    chosen = np.arange(n)[::7]
    ph.flags[chosen] = event.SURFACE_DETECT
    ph.last_hit_triangles[chosen] = chosen * 17 % 380000
    channel_of_triangle = np.asarray(geometry.solid_id_to_channel_index)[np.asarray(geometry.solid_id)]
    without = np.flatnonzero(channel_of_triangle < 0)
    assert len(without) > 0
    ph.last_hit_triangles[chosen[::3]] = without[(chosen[::3] * 31) % len(without)]
    return ph, chosen


# ---- the derivation itself, without a GPU ------------------------------------------------------------------------------------------
def test_derivation_of_the_expected_hits(oracle_mod, tiny_geometry, tiny_packed):
    """The expected side on a machine without a GPU: bomb(8193, 5) on tiny, seed 7, gives 188 hits on 52 channels in 2 launches."""
    want = expected_from_oracle(oracle_mod, tiny_geometry, tiny_packed, bomb(8193, 5), seed=7)
    assert want.nhits == 188 and want.launches == 2
    assert len(want.counts) == tiny_geometry.num_channels() and np.count_nonzero(want.counts) == 52
    assert int(want.counts.sum()) == want.nhits == len(want.hits) == len(want.hit_counters)
    assert np.array_equal(want.earliest == NO_HIT_TIME, want.counts == 0)
    assert (want.hits.flags & event.SURFACE_DETECT).all() and (want.hits.last_hit_triangles > -1).all()
    for c in np.flatnonzero(want.counts):
        on = want.hits.channel == c
        assert on.sum() == want.counts[c] and want.earliest[c] == want.hits.t[on].view(np.uint32).min()
    assert np.array_equal(want.hit_counters, want.counters[want.index]) and (want.hit_counters > 0).all()
    # a flagged photon is a hit only with a triangle, on a solid that has a channel
    channel_of_triangle = np.asarray(tiny_geometry.solid_id_to_channel_index)[np.asarray(tiny_geometry.solid_id)]
    without, with_channel = np.flatnonzero(channel_of_triangle < 0), np.flatnonzero(channel_of_triangle >= 0)
    assert len(without) > 0 and len(with_channel) > 0
    ph = bomb(4, 1)
    ph.flags[:] = [event.SURFACE_DETECT, event.SURFACE_DETECT, event.SURFACE_DETECT, event.SURFACE_ABSORB]
    ph.last_hit_triangles[:] = [without[0], -1, with_channel[5], with_channel[5]]
    index, hits, hit_counters, counts, earliest = derive_hits(tiny_geometry, ph, np.arange(4))
    assert index.tolist() == [2] and hits.channel.tolist() == [channel_of_triangle[with_channel[5]]] and hit_counters.tolist() == [2]
    assert counts.sum() == 1 and earliest[hits.channel[0]] == 0 and (np.delete(earliest, hits.channel[0]) == NO_HIT_TIME).all()
    # the pre-flagged input: some of its chosen photons are hits, some are not
    ph, chosen = preflagged(tiny_geometry)
    index = derive_hits(tiny_geometry, ph, np.zeros(len(ph)))[0]
    assert 0 < len(index) < len(chosen) and np.isin(index, chosen).all()


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
@gpu_test
@pytest.mark.parametrize('n', [1, 63, 64, 65, 4095, 4096, 4097, 8191, 8192, 8193, 12289])
def test_size_boundaries(gpu, oracle_mod, tiny, n):
    want, stats = fused(gpu, oracle_mod, tiny, bomb(n, 5), max_steps=100)
    if n < FEW:
        assert stats['launches'] == 1          # the tail kernel from step 0
    elif n > FEW:
        assert stats['launches'] >= 2          # per-step launches first
    if n >= 4095:
        assert want.nhits > 50
    assert alive(want.end) == 0


@gpu_test
@pytest.mark.parametrize('n', [12289, 8193])
@pytest.mark.parametrize('max_steps', [1, 2, 3])
def test_photons_alive_when_the_call_ends(gpu, oracle_mod, tiny, n, max_steps):
    """They come back through k_store_working (or from the tail kernel, entered on the last allowed steps of the smaller batch)
    and are read from the arrays by the pass."""
    want, stats = fused(gpu, oracle_mod, tiny, bomb(n, 5), max_steps=max_steps)
    if max_steps in (1, 3):
        assert alive(want.end) > 100
    if (n, max_steps) == (12289, 3):
        assert want.nhits > 100


@gpu_test
@pytest.mark.parametrize('id_base', [875000000, 2 ** 32 + 12345])
def test_photon_id_base(gpu, oracle_mod, tiny, id_base):
    """(the second: the 64-bit add of cm_rng_init(seed, id_base + photon_id, ...))"""
    want, stats = fused(gpu, oracle_mod, tiny, bomb(12289, 5), id_base=id_base)
    assert want.nhits > 50
    other = expected_from_oracle(oracle_mod, tiny[0], tiny[1], bomb(12289, 5), seed=7, id_base=0)
    assert not np.array_equal(other.end.flags, want.end.flags)        # (the id base does reach the streams)


@gpu_test
@pytest.mark.parametrize('n', [12289, 8000])
def test_incoming_draw_counters(gpu, oracle_mod, tiny, n):
    """Two steps, then the same GPUPhotons continued for 98 more by a second fused call: the oracle continued the same way."""
    ph = bomb(n, 5)
    gp = gpu.GPUPhotons(ph)
    first, _ = fused(gpu, oracle_mod, tiny, ph, max_steps=2, gp=gp, id_base=99)
    assert alive(first.end) > 100 and (first.counters > 0).any()
    second, _ = fused(gpu, oracle_mod, tiny, ph, max_steps=98, gp=gp, id_base=99, oracle_input=first.end, counters_in=first.counters)
    assert alive(second.end) == 0 and second.nhits > first.nhits and second.nhits > 50


@gpu_test
def test_the_c_export_the_benchmark_calls(gpu, oracle_mod, tiny):
    """chroma_propagate_hits itself (everything else reaches the kernels through chroma_propagate_opt), shaped as bench.py's
    run_step; then without the earliest-time array, and with the channel arrays alone."""
    from chroma_amd import _lib
    from chroma_amd.gpu.photon import GPUPhotonsSlice, _alloc_fields, _structure
    from chroma_amd.gpu.tools import empty
    geometry, packed, gg = tiny
    ctx = gpu.get_context()
    lib = ctx._lib
    ph, seed, id_base, n = bomb(12289, 5), 7, 3 * 12289, 12289
    want = expected_from_oracle(oracle_mod, geometry, packed, ph, seed, id_base)
    assert want.nhits > 50 and want.launches >= 2
    capacity = int(1.25 * want.nhits) + 1024

    def call(flat, with_earliest):
        gp = gpu.GPUPhotons(ph)
        s = _structure(gp)
        out = GPUPhotonsSlice(**_alloc_fields(capacity, ctx))
        dst, channels = _structure(out), empty(capacity, np.int32, ctx)
        counts, earliest = channel_arrays(gpu, gg)
        req = _lib.HitsRequest()
        req.detection_state = event.SURFACE_DETECT
        req.capacity = capacity
        if flat:
            req.dst = ctypes.pointer(dst)
            req.d_channels = channels.ptr
        req.d_hit_count = counts.ptr
        req.d_earliest_time_bits = earliest.ptr if with_earliest else None
        st, aborted = _lib.PropagateStats(), ctypes.c_int32(0)
        _lib.check(lib.chroma_propagate_hits(ctx.handle, gg.handle, ctypes.byref(s), n, 1, _lib.Rng(seed, id_base), 100, 0, 0, 0,
                                             ctypes.byref(st), ctypes.byref(aborted), ctypes.byref(req)))
        what = 'chroma_propagate_hits, flat hits %s, earliest %s' % (flat, with_earliest)
        assert_photons(gp, want, what)
        assert req.nhits == want.nhits and aborted.value == 0, what
        assert st.launches == want.launches, what
        assert np.array_equal(counts.get(), want.counts), what
        assert np.array_equal(earliest.get(), want.earliest if with_earliest else np.full(gg.nchannels, NO_HIT_TIME, np.uint32)), what
        if flat:
            w = slice(0, int(req.nhits))
            hits = GPUPhotonsSlice(pos=out.pos[w], dir=out.dir[w], pol=out.pol[w], wavelengths=out.wavelengths[w], t=out.t[w],
                                   last_hit_triangles=out.last_hit_triangles[w], flags=out.flags[w], weights=out.weights[w],
                                   evidx=out.evidx[w], rng_counters=out.rng_counters[w])
            assert_hits(*fetch(hits, channels[w]), want, what)

    call(True, True)
    call(True, False)
    call(False, True)


@gpu_test
@pytest.mark.parametrize('options', [dict(use_weights=True), dict(scatter_first=-1), dict(scatter_first=1), dict(exact=True)],
                         ids=['weights', 'scatter_first-1', 'scatter_first+1', 'exact'])
def test_options(gpu, oracle_mod, tiny, options):
    want, stats = fused(gpu, oracle_mod, tiny, bomb(12289, 5), **options)
    assert want.nhits > 50
    if options.get('use_weights'):
        assert stats['launches'] == 1 and (want.end.weights != 1.0).any()       # (with weights the reference runs one launch)


@gpu_test
def test_copies(gpu, oracle_mod, tiny):
    """ncopies=3 of 1000 photons: the oracle's input is the tiled batch, as k_init_queue lays the clones out."""
    ph = bomb(1000, 9)
    ph.evidx[:] = np.arange(1000) % 5
    want, stats = fused(gpu, oracle_mod, tiny, ph, ncopies=3)
    assert len(want.end) == 3000 and want.nhits > 10
    assert not np.array_equal(want.end.flags[:1000], want.end.flags[1000:2000])       # (clones draw from their own streams)


@gpu_test
def test_mixed_wavelengths_and_edge_inputs(gpu, oracle_mod, tiny):
    want, _ = fused(gpu, oracle_mod, tiny, bomb(12289, 3, wavelength=400.0, wavelength_hi=800.0))
    assert want.nhits > 50 and len(np.unique(want.hits.wavelengths)) > 50
    want, _ = fused(gpu, oracle_mod, tiny, _edge_photons(), max_steps=20)
    assert (want.end.flags & event.NAN_ABORT).any() and (want.end.flags[100:200] == event.BULK_ABSORB).all()


@gpu_test
@pytest.mark.parametrize('exact', [False, True], ids=['default', 'exact'])
@pytest.mark.parametrize('n', [8191, 8193, 20000])
def test_every_surface_model(gpu, oracle_mod, stress, n, exact):
    """All hits of this geometry fall on ONE channel: the one-atomic-per-wave path of k_finalize_hits' channel arrays."""
    want, stats = fused(gpu, oracle_mod, stress, bomb(n, 6, wavelength=350.0), seed=11, exact=exact)
    assert want.nhits > 100 and np.count_nonzero(want.counts) == 1
    if n == 20000:
        assert int(np.bitwise_or.reduce(want.end.flags)) & 0x3FE == 0x3FE and stats['launches'] >= 2


@gpu_test
def test_photons_that_were_terminal_before_the_call(gpu, oracle_mod, tiny):
    ph, chosen = preflagged(tiny[0])
    want, _ = fused(gpu, oracle_mod, tiny, ph, max_steps=20)
    was_hit = np.isin(chosen, want.index)
    assert was_hit.any() and (~was_hit).any()               # pre-flagged photons on both sides of the channel map
    assert (want.hit_counters == 0).any() and (want.hit_counters > 0).any()
    assert np.array_equal(want.end.dir[chosen], ph.dir[chosen])


@gpu_test
def test_capacity(gpu, oracle_mod, tiny):
    """Room for 1 hit, for all but one, and for exactly all of them: the same result set."""
    ph = bomb(12289, 5)
    want = expected_from_oracle(oracle_mod, tiny[0], tiny[1], ph, seed=7)
    assert want.nhits > 50
    for capacity in (1, want.nhits - 1, want.nhits):
        fused(gpu, oracle_mod, tiny, ph, capacity=capacity, want=want, what='capacity %d of %d' % (capacity, want.nhits))


@gpu_test
def test_a_sequence_of_calls_on_one_context(gpu, oracle_mod, tiny_geometry, tiny_packed):
    """What the epoch stamp exists for.  A context of its own, so that the final-record buffer starts empty whatever ran before:
    20000 photons; a plain propagate; 9000 OTHER photons (stale records of the first call under and beyond their ids, its tail
    stamps in the buffer); 30000 (the buffer is reallocated, the epoch restarts); 20000 again; 8000 (tail only); 12289 cut off
    after one step; and the first batch again, which must give the first call's result bit for bit."""
    from chroma_amd.gpu.tools import Context
    ctx = Context(0)
    with ctx.bound():
        where = (tiny_geometry, tiny_packed, gpu.GPUDetector(tiny_geometry))
        first, _ = fused(gpu, oracle_mod, where, bomb(20000, 61), what='call 1')
        assert first.nhits > 50
        plain = gpu.GPUPhotons(bomb(15000, 62))
        plain.propagate(where[2], gpu.get_rng_states(64, seed=7), max_steps=100)
        for k, (n, seed, max_steps) in enumerate([(9000, 63, 100), (30000, 64, 100), (20000, 65, 100), (8000, 66, 100), (12289, 67, 1)]):
            want, stats = fused(gpu, oracle_mod, where, bomb(n, seed), max_steps=max_steps, what='call %d' % (k + 2))
            assert (stats['launches'] == 1) == (n < FEW or max_steps == 1)
        fused(gpu, oracle_mod, where, bomb(20000, 61), want=first, what='call 7, the first batch again')
    ctx.synchronize()       # (not shut down: the geometry made on it is freed whenever the garbage collector gets to it)


@gpu_test
def test_no_step_and_no_photon(gpu, oracle_mod, tiny):
    """max_steps=0 with a hits request means propagate(max_steps=0) + get_flat_hits: the photons detected before the call are its
    hits, the channel arrays are filled, the photon arrays stay as they are.  No photon: an empty set and CHROMA_OK."""
    from chroma_amd import _lib
    geometry, packed, gg = tiny
    ph, chosen = preflagged(geometry)
    want, stats = fused(gpu, oracle_mod, tiny, ph, max_steps=0)
    assert 0 < want.nhits < len(chosen) and want.launches == 0
    assert_bit_exact(want.end, ph, 'the oracle at max_steps=0')
    # ... and without a request nothing happens at all
    gp = gpu.GPUPhotons(ph)
    gp.propagate(gg, _lib.Rng(7, 0), max_steps=0)
    assert_photons(gp, want, 'propagate(max_steps=0)')
    empty_batch = gpu.GPUPhotons(Photons())
    counts, earliest = channel_arrays(gpu, gg)
    stats = {}
    hits = empty_batch.propagate_hits(gg, _lib.Rng(7, 0), max_steps=100, channel_arrays=(counts, earliest), stats=stats)
    assert len(hits) == 0 and stats['nhits'] == 0 and len(empty_batch.get()) == 0
    assert not counts.get().any() and (earliest.get() == NO_HIT_TIME).all()
