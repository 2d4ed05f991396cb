"""Two host threads on ONE context: every call that uses the context's scratch state runs under its call lock.

include/chroma_hip.h promises that calls on one context run one at a time and that two threads may share a handle.  The calls
below meet in the same scratch words: a propagate_hits of 4096 photons ends in k_tail_coop with k_finalize_hits beside it on
the auxiliary stream, both writing the hit count and the abort bits, and get_flat_hits / count_photon_hits / select clear, bump
and read back that hit count for a photon set of their own.  Run side by side, each must give what it gives alone.

The first test checks that this HOLDS.  It is not a reproducer: without the lock the two threads race, but whether a given run
of a few dozen rounds loses that race is chance, so a build without the lock may well pass it.  The second test is
deterministic: a set_walk on one thread between two calls of another changes the second call and not the first.
"""
import ctypes
import threading

import numpy as np
import pytest

from chroma_amd import event
from conftest import bomb
from test_gpu_parity import assert_bit_exact

pytestmark = pytest.mark.gpu

ROUNDS = 40
A_PHOTONS = 4096        # below the 8192 photons at which a call hands its photons to the tail kernel: the whole call is the tail
B_PHOTONS = 1001


@pytest.fixture(scope='module')
def gpu():
    from chroma_amd import gpu as g
    ctx = g.create_cuda_context(0)
    yield g
    ctx.pop()


def ordered(p, with_channel):
    """``p`` in an order of its own fields (flat hits and selections come in no particular order)."""
    keys = [p.dir[:, 0].view(np.uint32), p.dir[:, 1].view(np.uint32), p.pol[:, 0].view(np.uint32), p.pos[:, 0].view(np.uint32),
            p.pos[:, 1].view(np.uint32), p.wavelengths.view(np.uint32), p.t.view(np.uint32), p.last_hit_triangles, p.flags]
    return p[np.lexsort(keys + ([p.channel] if with_channel else []))]


def run_a(g, gg, photons, stats=None):
    """The fused call on a fresh copy of ``photons``: (arrays, draw counters, flat hits in order, hit count)."""
    stats = {} if stats is None else stats
    p = g.GPUPhotons(photons)
    hits = p.propagate_hits(gg, g.get_rng_states(64, seed=7), max_steps=100, stats=stats)
    return p.get(), p.rng_counters.get(), ordered(hits, True), stats['nhits']


def run_b(g, gg, pb):
    """The hit and count calls on the propagated set ``pb``: (flat hits in order, hit count, the detected photons in order)."""
    from chroma_amd.gpu.photon import _structure
    ctx = g.get_context()
    flat = ordered(pb.get_flat_hits(gg), True)
    count = ctypes.c_uint32(0xFFFFFFFF)
    src = _structure(pb)
    rc = ctx._lib.chroma_count_photon_hits(ctx.handle, gg.handle, 0, len(pb), int(event.SURFACE_DETECT), ctypes.byref(src), ctypes.byref(count))
    assert rc == 0
    return flat, count.value, ordered(pb.select(event.SURFACE_DETECT).get(), False)


def same_a(got, want):
    assert_bit_exact(got[0], want[0], 'photon arrays')
    assert np.array_equal(got[1], want[1]), 'draw counters'
    assert got[3] == want[3] == len(got[2]), 'hit count %d, %d flat hits, alone %d' % (got[3], len(got[2]), want[3])
    assert_bit_exact(got[2], want[2], 'flat hits')
    assert np.array_equal(got[2].channel, want[2].channel), 'channels of the flat hits'


def same_b(got, want):
    assert got[1] == want[1] == len(got[0]), 'count_photon_hits %d, %d flat hits, alone %d' % (got[1], len(got[0]), want[1])
    assert_bit_exact(got[0], want[0], 'flat hits')
    assert np.array_equal(got[0].channel, want[0].channel), 'channels of the flat hits'
    assert len(got[2]) == len(want[2]), 'select: %d photons, alone %d' % (len(got[2]), len(want[2]))
    assert_bit_exact(got[2], want[2], 'selected photons')


def test_hit_calls_beside_a_fused_call(gpu, tiny_geometry):
    g = gpu
    ctx = g.get_context()
    gg = g.GPUDetector(tiny_geometry)
    photons_a = bomb(A_PHOTONS, 21)
    photons_b = bomb(B_PHOTONS, 22)
    # (some detected before the call as well, on triangles all over the mesh)
    photons_b.flags[::7] = event.SURFACE_DETECT
    photons_b.last_hit_triangles[::7] = np.arange(B_PHOTONS)[::7] * 17 % len(tiny_geometry.mesh.triangles)
    pb = g.GPUPhotons(photons_b)
    pb.propagate(gg, g.get_rng_states(64, seed=8), max_steps=100)
    want_a, want_b = run_a(g, gg, photons_a), run_b(g, gg, pb)
    assert want_a[3] > 0 and want_b[1] > 0 and len(want_b[2]) >= len(want_b[0]) > 0          # (both sides have hits to lose)
    same_a(run_a(g, gg, photons_a), want_a)          # (and give them again, alone)
    same_b(run_b(g, gg, pb), want_b)

    failures, stop = [], threading.Event()

    def worker(name, run, same, want):
        with ctx.bound():
            for k in range(ROUNDS):
                if stop.is_set():
                    return
                try:
                    same(run(), want)
                except Exception as e:          # (the first mismatch, or a failed call, ends this thread; nothing is tried again)
                    failures.append('thread %s, round %d: %s: %s' % (name, k, type(e).__name__, e))
                    stop.set()
                    return

    threads = [threading.Thread(target=worker, args=('A', lambda: run_a(g, gg, photons_a), same_a, want_a)),
               threading.Thread(target=worker, args=('B', lambda: run_b(g, gg, pb), same_b, want_b))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not failures, '; '.join(failures)


def test_set_walk_changes_only_calls_that_start_after_it(gpu, tiny_geometry):
    """The default walk and the exact walk agree on this geometry photon for photon; what tells them apart is the work
    the kernels count, so the calls count: the exact walk makes the reference's very tests, the same number every time,
    the default walk fewer triangle tests over a different tree (tests/test_gpu_literal.py)."""
    g = gpu
    ctx = g.get_context()
    gg = g.GPUDetector(tiny_geometry)
    photons = bomb(A_PHOTONS, 23)
    WORK = ('photon_steps', 'nodes_visited', 'triangles_tested')

    def call():
        stats = {}
        out = run_a(g, gg, photons, stats)
        return out, tuple(stats[k] for k in WORK)

    default_walk = ctx.walk
    ctx.set_counting(True)
    try:
        ctx.read_stats()          # (whatever earlier calls counted)
        want_default, work_default = call()
        ctx.set_walk('exact')
        want_exact, work_exact = call()
        ctx.set_walk(default_walk)
        def is_default(work):
            return work[0] == work_exact[0] and work[1] != work_exact[1] and 0 < work[2] < work_exact[2]

        assert work_exact[0] > 0 and is_default(work_default), 'the counts do not tell the walks apart: %r, exact %r' % (work_default, work_exact)

        first_done, walk_set, got = threading.Event(), threading.Event(), {}

        def caller():
            with ctx.bound():
                try:
                    got['first'] = call()
                finally:
                    first_done.set()
                walk_set.wait()
                got['second'] = call()

        def setter():
            with ctx.bound():
                first_done.wait()
                try:
                    ctx.set_walk('exact')
                finally:
                    walk_set.set()

        threads = [threading.Thread(target=caller), threading.Thread(target=setter)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        same_a(got['first'][0], want_default)
        same_a(got['second'][0], want_exact)
        assert is_default(got['first'][1]), 'the call before set_walk: %r, the default walk alone %r, the exact walk %r' % (got['first'][1], work_default, work_exact)
        assert got['second'][1] == work_exact, 'the call after set_walk: %r, the exact walk alone %r' % (got['second'][1], work_exact)
    finally:
        ctx.set_walk(default_walk)
        ctx.set_counting(False)
