"""Photon tracks recorded on the device (GPUPhotons.propagate_tracks, chroma_propagate_tracks) on a real MI355X: bit for
bit the reference's tracking loop -- the CPU oracle driven one step per launch -- and today's propagate(track=True), at the
sizes where the append, the scan and the scatter can go wrong, with every option, and through Simulation and chroma-sim."""
import os
import re

import numpy as np
import pytest

from chroma_amd import event
from chroma_amd.event import Photons
from chroma_amd.tracks import PhotonTracks
from conftest import ROOT, make_stress_geometry, bomb
from test_tracks_host import assert_bit_exact, assert_tracks_equal, oracle_steps

pytestmark = pytest.mark.gpu


def _source_constant(path, name):
    text = open(os.path.join(ROOT, 'chroma_amd', 'csrc', path)).read()
    return int(re.search(r'^#define\s+%s\s+(\d+)' % name, text, flags=re.M).group(1))


PHYS_BLOCK = _source_constant('kernel_physics.h', 'PHYS_BLOCK')
COPY_SPAN = _source_constant('device_common.h', 'COPY_ITEMS') * 256
# the sizes the issue names, and the block sizes of the kernels around the recorder with their neighbours
SIZES = sorted({0, 1, 63, 64, 65, 255, 256, 257, 4097} | {b + d for b in (PHYS_BLOCK, COPY_SPAN) for d in (-1, 0, 1)})


@pytest.fixture(scope='module')
def gpu():
    from chroma_amd import gpu as g
    ctx = g.create_cuda_context(0)
    yield g
    ctx.pop()


@pytest.fixture(scope='module')
def stress(gpu):
    from chroma_amd.gpu.geometry import pack_geometry
    geo = make_stress_geometry()
    return geo, pack_geometry(geo), gpu.GPUDetector(geo)


def device_tracks(gpu, gg, photons, seed, max_steps, ncopies=1, **kw):
    gp = gpu.GPUPhotons(photons, ncopies=ncopies)
    tracks = gp.propagate_tracks(gg, gpu.get_rng_states(64, seed=seed), max_steps=max_steps, **kw)
    return gp, tracks


def test_core_oracle_and_todays_tracking(gpu, oracle_mod, stress):
    geo, pk, gg = stress
    ph = bomb(300, 12, wavelength=350.0)
    gp, tracks = device_tracks(gpu, gg, ph, seed=2, max_steps=8)
    ids, rows, final, ctr = oracle_steps(oracle_mod, pk, ph, seed=2, max_steps=8)
    assert_tracks_equal(tracks, PhotonTracks.from_steps(ids, rows, 300), 'against the oracle')
    assert_bit_exact(gp.get(), final, 'final arrays')
    assert np.array_equal(gp.rng_counters.get(), ctr)
    # every terminal flag and surface model is reached, photons end at every step
    assert int(np.bitwise_or.reduce(tracks.photons.flags)) & 0x3FE == 0x3FE
    assert len(np.unique(tracks.steps_taken)) > 3
    # today's tracking mode, regrouped
    gp2 = gpu.GPUPhotons(ph)
    ids2, rows2 = gp2.propagate(gg, gpu.get_rng_states(64, seed=2), max_steps=8, track=True)
    assert_tracks_equal(tracks, PhotonTracks.from_steps(ids2, rows2, 300), 'against propagate(track=True)')
    assert_bit_exact(gp.get(), gp2.get(), 'final arrays against propagate(track=True)')
    assert np.array_equal(gp.rng_counters.get(), gp2.rng_counters.get())


_edge_reference = {}


def edge_reference(oracle_mod, pk, n):
    """(photons, oracle step lists of three steps) for ``n`` photons, made once per size: the lists of a call of fewer steps
    are their first entries."""
    if n not in _edge_reference:
        ph = bomb(n, 1000 + n, wavelength=350.0)
        ids, rows, _, _ = oracle_steps(oracle_mod, pk, ph, seed=7, max_steps=3) if n else ([], [], None, None)
        _edge_reference[n] = (ph, ids, rows)
    return _edge_reference[n]


@pytest.mark.parametrize('max_steps', [0, 1, 3])
@pytest.mark.parametrize('n', SIZES)
def test_size_edges(gpu, oracle_mod, stress, n, max_steps):
    geo, pk, gg = stress
    ph, ids, rows = edge_reference(oracle_mod, pk, n)
    gp, tracks = device_tracks(gpu, gg, ph, seed=7, max_steps=max_steps)
    want = PhotonTracks.from_steps(ids[:max_steps + 1], rows[:max_steps + 1], n)
    assert_tracks_equal(tracks, want, '%d photons, %d steps' % (n, max_steps))
    assert len(tracks) == n
    if n and max_steps:
        assert tracks.steps_taken.min() >= 1
        last = tracks.photons[(tracks.offsets[1:] - 1).astype(np.int64)]
        assert_bit_exact(gp.get(), last, 'final arrays are the last rows')
    else:
        assert_bit_exact(gp.get(), ph, 'no step: the photons are untouched')


def test_terminal_at_entry(gpu, oracle_mod, stress):
    geo, pk, gg = stress
    ph = bomb(600, 31, wavelength=350.0)
    rng_states = gpu.get_rng_states(64, seed=9)
    gp = gpu.GPUPhotons(ph)
    gp.propagate(gg, rng_states, max_steps=2)
    mid, mid_ctr = gp.get(), gp.rng_counters.get()
    cur, ctr, _ = oracle_mod.propagate(pk, ph, seed=9, max_steps=2, nthreads=8)
    assert_bit_exact(mid, cur, 'the two steps before')
    ended = (mid.flags & event.TERMINAL_MASK) != 0
    assert 50 < ended.sum() < 550
    tracks = gp.propagate_tracks(gg, rng_states, max_steps=4)
    ids, rows, final, final_ctr = oracle_steps(oracle_mod, pk, cur, seed=9, max_steps=4, rng_counters=ctr)
    assert_tracks_equal(tracks, PhotonTracks.from_steps(ids, rows, 600), 'continued from the oracle\'s counters')
    assert np.array_equal(tracks.steps_taken[ended], np.ones(ended.sum(), dtype=np.int64))
    for i in np.flatnonzero(ended):
        assert_bit_exact(tracks[i][0:1], mid[i:i + 1], 'terminal photon %d, row 0' % i)
        assert_bit_exact(tracks[i][1:2], mid[i:i + 1], 'terminal photon %d, row 1' % i)
    assert_bit_exact(gp.get(), final, 'final arrays')
    assert np.array_equal(gp.rng_counters.get(), final_ctr)
    assert np.array_equal(gp.rng_counters.get()[ended], mid_ctr[ended])
    # no step at all: one row each, terminal or not
    gp0, tracks0 = device_tracks(gpu, gg, mid, seed=9, max_steps=0)
    assert np.array_equal(tracks0.offsets, np.arange(601, dtype=np.uint64))
    assert_bit_exact(tracks0.photons, mid, 'max_steps = 0')


@pytest.mark.parametrize('variant', ['ncopies', 'weights', 'exact'])
def test_option_variants(gpu, oracle_mod, stress, variant):
    geo, pk, gg = stress
    ph = bomb(400, 41, wavelength=350.0)
    kw, okw, ncopies, expanded = {}, {}, 1, ph
    if variant == 'ncopies':
        ncopies, expanded = 3, Photons.join([ph, ph, ph])
    elif variant == 'weights':
        kw = okw = dict(use_weights=True, scatter_first=1)
    else:
        kw = dict(exact=True)
    gp, tracks = device_tracks(gpu, gg, ph, seed=13, max_steps=6, ncopies=ncopies, **kw)
    ids, rows, final, ctr = oracle_steps(oracle_mod, pk, expanded, seed=13, max_steps=6, **okw)
    assert_tracks_equal(tracks, PhotonTracks.from_steps(ids, rows, len(expanded)), variant)
    assert_bit_exact(gp.get(), final, variant + ', final arrays')
    assert np.array_equal(gp.rng_counters.get(), ctr)
    if variant == 'ncopies':
        # the copies start alike and go their own ways
        assert_bit_exact(tracks[5][0:1], tracks[405][0:1], 'row 0 of a photon and its copy')
        assert not np.array_equal(tracks.steps_taken[:400], tracks.steps_taken[400:800])
    if variant == 'weights':
        assert (tracks.photons.weights != 1.0).any()


def test_across_the_launch_threshold(gpu, oracle_mod, tiny_geometry, tiny_packed):
    """20 000 photons fall below the reference's 8192-photon threshold within the ten steps: the untracked propagate stops
    re-normalising there, tracking mode (one launch per step) never does."""
    gg = gpu.GPUDetector(tiny_geometry)
    ph = oracle_mod.generate_bomb(20000, seed=5)
    gp, tracks = device_tracks(gpu, gg, ph, seed=3, max_steps=10)
    ids, rows, final, ctr = oracle_steps(oracle_mod, tiny_packed, ph, seed=3, max_steps=10)
    assert len(ids[1]) >= 8192 > len(ids[-1]) > 0, [len(i) for i in ids]
    assert_tracks_equal(tracks, PhotonTracks.from_steps(ids, rows, 20000), 'tiny, 20 000 photons')
    assert_bit_exact(gp.get(), final, 'final arrays')
    assert np.array_equal(gp.rng_counters.get(), ctr)


def test_no_state_left_behind(gpu, stress):
    geo, pk, gg = stress
    ph = bomb(3000, 51, wavelength=350.0)
    gp1, first = device_tracks(gpu, gg, ph, seed=17, max_steps=5)
    gp2, second = device_tracks(gpu, gg, ph, seed=17, max_steps=5)
    assert_tracks_equal(second, first, 'two tracking calls in a row')
    assert_bit_exact(gp2.get(), gp1.get(), 'their final arrays')
    # an untracked call after a tracking call, against the same call on a context that never tracked
    gp3 = gpu.GPUPhotons(ph)
    gp3.propagate(gg, gpu.get_rng_states(64, seed=17), max_steps=20)
    after, after_ctr = gp3.get(), gp3.rng_counters.get()
    fresh = gpu.tools.Context(gpu.get_context().device_id)
    with fresh.bound():
        gg2 = gpu.GPUDetector(geo)
        gp4 = gpu.GPUPhotons(ph)
        gp4.propagate(gg2, gpu.get_rng_states(64, seed=17), max_steps=20)
        assert_bit_exact(after, gp4.get(), 'propagate after a tracking call')
        assert np.array_equal(after_ctr, gp4.rng_counters.get())


def _tracks_call(gpu, gg, gp, seed, max_steps, tail=-1):
    """chroma_propagate_tracks itself, with the options' tail field: returns the error message, or None (the rows released)."""
    import ctypes
    from chroma_amd import _lib
    from chroma_amd.gpu.photon import _structure
    ctx = gpu.get_context()
    s, opt = _structure(gp), _lib.PropagateOptions(max_steps, tail=tail)
    handle, nrows, aborted = ctypes.c_void_p(), ctypes.c_uint64(0), ctypes.c_int32(0)
    rc = ctx._lib.chroma_propagate_tracks(ctx.handle, gg.handle, ctypes.byref(s), len(gp), 1, _lib.Rng(seed, 0), ctypes.byref(opt), None,
                                          ctypes.byref(aborted), ctypes.byref(handle), ctypes.byref(nrows))
    if rc != 0:
        assert handle.value is None and nrows.value == 0
        return ctx._lib.chroma_last_error().decode()
    _lib.check(ctx._lib.chroma_tracks_destroy(ctx.handle, handle))
    return None


def test_fused_tail_is_refused(gpu, stress):
    from chroma_amd import _lib
    geo, pk, gg = stress
    ctx = gpu.get_context()
    ph = bomb(100, 61, wavelength=350.0)
    gp = gpu.GPUPhotons(ph)
    # as the context's setting ...
    _lib.check(ctx._lib.chroma_set_tail(ctx.handle, 2))
    try:
        with pytest.raises(_lib.ChromaError, match='fused'):
            gp.propagate_tracks(gg, gpu.get_rng_states(64, seed=1), max_steps=3)
        # ... which the call's own options override, as in every propagate call
        assert _tracks_call(gpu, gg, gpu.GPUPhotons(ph), 1, 3, tail=1) is None
    finally:
        _lib.check(ctx._lib.chroma_set_tail(ctx.handle, 0))
    assert_bit_exact(gp.get(), ph, 'a refused call touches nothing')
    # ... and as the call's option, the context in its default mode (the cooperative tail)
    assert 'fused' in _tracks_call(gpu, gg, gp, 1, 3, tail=2)
    assert_bit_exact(gp.get(), ph, 'a refused call touches nothing')
    # more rows than a call holds: refused before anything runs
    with pytest.raises(_lib.ChromaError, match='rows'):
        gp.propagate_tracks(gg, gpu.get_rng_states(64, seed=1), max_steps=2 ** 31 - 2)
    assert_bit_exact(gp.get(), ph, 'a refused call touches nothing')


def test_split_loop_whatever_the_tail_mode(gpu, oracle_mod, stress):
    """The context's default tail (the cooperative tail kernel, which takes the last < 8192 photons of an untracked call) and
    the options' COOP are both taken as SPLIT: 300 photons are below that threshold from the first step on, and every step is
    a launch of its own all the same -- `launches` counts the steps that had photons, and the rows are the oracle's."""
    geo, pk, gg = stress
    ph = bomb(300, 12, wavelength=350.0)
    ids, rows, final, ctr = oracle_steps(oracle_mod, pk, ph, seed=2, max_steps=8)
    stats = {}
    gp, tracks = device_tracks(gpu, gg, ph, seed=2, max_steps=8, stats=stats)
    assert stats['launches'] == len(ids) - 1 >= 4
    assert_tracks_equal(tracks, PhotonTracks.from_steps(ids, rows, 300), 'default tail mode')
    gp2 = gpu.GPUPhotons(ph)
    assert _tracks_call(gpu, gg, gp2, 2, 8, tail=0) is None
    assert_bit_exact(gp2.get(), final, 'options.tail = COOP')
    assert np.array_equal(gp2.rng_counters.get(), ctr)


def test_row_limit_between_steps_leaves_the_photons_consistent(gpu, oracle_mod, stress, monkeypatch):
    """A call that runs out of room for the next step's rows (here: the caller's row limit; the path is the one a failed
    allocation takes) stops BETWEEN two steps: the error, no tracks, and the photons as the steps taken left them, draw
    counters included -- so that going on from there gives the rest of the same tracks."""
    from chroma_amd import _lib
    geo, pk, gg = stress
    n = 600
    ph = bomb(n, 71, wavelength=350.0)
    ids, rows, final, ctr = oracle_steps(oracle_mod, pk, ph, seed=19, max_steps=6)
    assert len(ids) >= 5 and len(ids[3]) > 0
    # room for rows 0 and the rows of steps 0 and 1, not for those of step 2
    limit = n + len(ids[1]) + len(ids[2]) + len(ids[3]) - 1
    rng_states = gpu.get_rng_states(64, seed=19)
    gp = gpu.GPUPhotons(ph)
    monkeypatch.setenv('CHROMA_TRACKS_MAX_ROWS', str(limit))
    with pytest.raises(_lib.ChromaError, match='2 steps were taken'):
        gp.propagate_tracks(gg, rng_states, max_steps=6)
    two, two_ctr = gp.get(), gp.rng_counters.get()
    _, _, want2, ctr2 = oracle_steps(oracle_mod, pk, ph, seed=19, max_steps=2)
    assert_bit_exact(two, want2, 'after the failed call: two steps taken')
    assert np.array_equal(two_ctr, ctr2)
    # the least a call records is known beforehand: refused with nothing touched
    monkeypatch.setenv('CHROMA_TRACKS_MAX_ROWS', str(2 * n - 1))
    with pytest.raises(_lib.ChromaError, match='at least'):
        gp.propagate_tracks(gg, rng_states, max_steps=6)
    assert_bit_exact(gp.get(), two, 'a refused call touches nothing')
    # going on without the limit: the remaining four steps of the same photons
    monkeypatch.delenv('CHROMA_TRACKS_MAX_ROWS')
    rest = gp.propagate_tracks(gg, rng_states, max_steps=4)
    ids4, rows4, final4, ctr4 = oracle_steps(oracle_mod, pk, want2, seed=19, max_steps=4, rng_counters=ctr2)
    assert_tracks_equal(rest, PhotonTracks.from_steps(ids4, rows4, n), 'the steps after the failed call')
    assert_bit_exact(gp.get(), final, 'final arrays')
    assert_bit_exact(final4, final, 'the oracle, continued the same way')
    assert np.array_equal(gp.rng_counters.get(), ctr)


def test_simulation_device_tracks(gpu, tiny_geometry):
    from chroma_amd.sim import Simulation
    events = [bomb(n, 200 + n) for n in (700, 1, 4096)]
    out = {}
    for mode in (True, 'device'):
        sim = Simulation(tiny_geometry, geant4_processes=0, seed=5, photon_tracking=mode)
        out[mode] = list(sim.simulate([Photons.join([e]) for e in events], keep_photons_end=True, max_steps=20))
    assert [len(ev.photon_tracks) for ev in out['device']] == [700, 1, 4096]
    for host, dev in zip(out[True], out['device']):
        assert isinstance(dev.photon_tracks, PhotonTracks) and len(host.photon_tracks) == len(dev.photon_tracks)
        assert_bit_exact(dev.photons_end, host.photons_end, 'event %d, final photons' % host.id)
        assert int(dev.photon_tracks.offsets[-1]) == sum(len(t) for t in host.photon_tracks)
        for i, (a, b) in enumerate(zip(dev.photon_tracks, host.photon_tracks)):
            assert_bit_exact(a, b, 'event %d, photon %d' % (host.id, i))
        assert len(dev.flat_hits) == len(host.flat_hits)


def test_cli_device_tracks(gpu, tmp_path):
    from chroma_amd import cli
    files = {}
    for flag in ('--track', '--device-tracks'):
        files[flag] = str(tmp_path / (flag.strip('-') + '.npz'))
        assert cli.main(['@chroma_amd.demo.tiny', '-n', '2', '--nphotons', '900', '-s', '4', '--max-steps', '15', flag,
                         '-o', files[flag]]) == 0
    host, dev = np.load(files['--track']), np.load(files['--device-tracks'])
    assert sorted(host.files) == sorted(dev.files)
    keys = [k for k in host.files if '/track/' in k]
    assert len(keys) == 2 * 5
    for k in host.files:
        a, b = host[k], dev[k]
        assert a.dtype == b.dtype and a.shape == b.shape, (k, a.dtype, b.dtype, a.shape, b.shape)
        assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b), k
