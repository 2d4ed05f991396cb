"""PhotonTracks (chroma_amd/tracks.py) on the host: from_steps against the per-row loop of Simulation's tracking mode, the
sequence behaviour, and the properties of a track set built from the CPU oracle driven one step per launch."""
import numpy as np
import pytest

from chroma_amd import event
from chroma_amd.event import Photons
from chroma_amd.tracks import PhotonTracks
from conftest import make_stress_geometry, bomb

FIELDS = ('flags', 'last_hit_triangles', 'pos', 'dir', 'pol', 't', 'wavelengths', 'weights', 'evidx')


def assert_bit_exact(got, want, what=''):
    assert len(got) == len(want), '%s: %d rows, expected %d' % (what, len(got), len(want))
    for name in FIELDS:
        a, b = getattr(got, name), getattr(want, name)
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name, a.dtype, b.dtype, a.shape, b.shape)
        same = (a.view(np.uint32) == b.view(np.uint32)) if a.dtype == np.float32 else (a == b)
        assert same.all(), '%s: %s differs in %d of %d rows (first at %s)' % (
            what, name, np.count_nonzero(~same.reshape(len(a), -1).all(axis=1)), len(a), np.argwhere(~same)[0])


def assert_tracks_equal(got, want, what=''):
    assert got.offsets.dtype == np.uint64 and np.array_equal(got.offsets, want.offsets), '%s: offsets differ' % what
    assert_bit_exact(got.photons, want.photons, what)


def oracle_steps(oracle_mod, packed, photons, seed, max_steps, rng_counters=None, use_weights=False, scatter_first=0):
    """The reference's tracking loop (chroma/gpu/photon.py:218-238) on the CPU oracle: one launch of one step at a time.
    Returns (step_photon_ids, step_photons, final photons, final draw counters) in the shape of propagate(track=True)."""
    n = len(photons)
    queue = np.arange(n)
    ids, rows, cur, ctr = [queue], [photons[queue]], photons, rng_counters
    for k in range(max_steps):
        cur, ctr, _ = oracle_mod.propagate(packed, cur, seed=seed, max_steps=1, rng_counters=ctr, use_weights=use_weights,
                                           scatter_first=scatter_first if k == 0 else 0, nthreads=8)
        ids.append(queue)
        rows.append(cur[queue])
        queue = queue[(cur.flags[queue] & event.TERMINAL_MASK) == 0]
        if len(queue) == 0:
            break
    return ids, rows, cur, ctr


def naive_tracks(step_ids_list, step_photons_list, nphotons):
    """The loop of Simulation._simulate_batch for one event that holds every photon: an append per (photon, step)."""
    tracks = [[] for _ in range(nphotons)]
    for step_ids, step_photons in zip(step_ids_list, step_photons_list):
        for k, pid in enumerate(step_ids):
            tracks[pid].append(step_photons[np.array([k])])
    return [Photons.join(t) if t else Photons() for t in tracks]


def synthetic_steps(nphotons, nsteps, seed, never=()):
    """Step lists with shuffled queue order: photon i ends after i % (nsteps + 1) steps; those in ``never`` are in no list."""
    rng = np.random.default_rng(seed)
    alive = np.array([i for i in range(nphotons) if i not in never], dtype=np.int64)
    ids, rows = [], []
    for k in range(nsteps + 1):
        q = rng.permutation(alive)
        ids.append(q.astype(np.uint32))
        m = len(q)
        p = Photons(rng.normal(size=(m, 3)), rng.normal(size=(m, 3)), rng.normal(size=(m, 3)), rng.uniform(300, 600, m),
                    t=np.full(m, float(k)) + q / 1000.0, last_hit_triangles=rng.integers(-1, 50, m),
                    flags=rng.integers(0, 1 << 12, m), weights=rng.uniform(0, 1, m), evidx=q % 3)
        rows.append(p)
        alive = np.array([i for i in alive if i % (nsteps + 1) > k], dtype=np.int64)
    return ids, rows


@pytest.mark.parametrize('nphotons,never', [(0, ()), (1, ()), (1, (0,)), (7, ()), (7, (2, 6))])
def test_from_steps_equals_the_per_row_loop(nphotons, never):
    ids, rows = synthetic_steps(nphotons, 4, seed=nphotons + len(never), never=never)
    tracks = PhotonTracks.from_steps(ids, rows, nphotons)
    want = naive_tracks(ids, rows, nphotons)
    assert len(tracks) == nphotons == len(want)
    for i in range(nphotons):
        assert_bit_exact(tracks[i], want[i], 'photon %d' % i)
        if i in never:
            assert len(tracks[i]) == 0
        else:
            # rows in step order: the time of the synthetic rows is step + id / 1000
            assert np.array_equal(tracks[i].t, (np.arange(i % 5 + 1) + np.float64(i) / 1000.0).astype(np.float32))
    assert tracks.offsets.dtype == np.uint64 and len(tracks.offsets) == nphotons + 1
    steps = np.array([-1 if i in never else i % 5 for i in range(nphotons)], dtype=np.int64)
    assert np.array_equal(tracks.steps_taken, steps)
    assert int(tracks.offsets[-1]) == len(tracks.photons) == sum(len(i) for i in ids)


def test_from_steps_without_any_step():
    tracks = PhotonTracks.from_steps([], [], 3)
    assert len(tracks) == 3 and all(len(t) == 0 for t in tracks) and np.array_equal(tracks.steps_taken, [-1, -1, -1])
    assert len(PhotonTracks.from_steps([], [], 0)) == 0


def test_sequence_behaviour():
    ids, rows = synthetic_steps(7, 4, seed=3, never=(2,))
    tracks = PhotonTracks.from_steps(ids, rows, 7)
    assert len(tracks) == 7
    assert_bit_exact(tracks[-1], tracks[6], 'negative index')
    assert_bit_exact(tracks[-7], tracks[0], 'negative index')
    for bad in (7, -8):
        with pytest.raises(IndexError):
            tracks[bad]
    listed = list(tracks)
    assert len(listed) == 7
    for i, t in enumerate(listed):
        assert isinstance(t, Photons)
        assert_bit_exact(t, tracks[i], 'iteration')
    # a track is a view of the flat arrays, not a copy
    assert np.shares_memory(tracks[3].pos, tracks.photons.pos)
    # the empty track: no rows, and slices of it are empty too
    empty = tracks[2]
    assert len(empty) == 0 and len(empty[0:5]) == 0 and len(empty[::-1]) == 0 and empty.pos.shape == (0, 3)
    # slices of the sequence
    part = tracks[1:4]
    assert isinstance(part, PhotonTracks) and len(part) == 3 and int(part.offsets[0]) == 0
    for i in range(3):
        assert_bit_exact(part[i], tracks[1 + i], 'slice')
    assert len(tracks[5:2]) == 0 and len(tracks[7:]) == 0
    assert [len(t) for t in tracks[::2]] == [len(tracks[i]) for i in (0, 2, 4, 6)]
    assert_tracks_equal(tracks.cut(0, 7), tracks, 'cut of everything')
    with pytest.raises(ValueError):
        PhotonTracks(np.array([0, 2, 3]), tracks.photons)


def test_oracle_track_set_properties(oracle_mod):
    from chroma_amd.gpu.geometry import pack_geometry
    geo = make_stress_geometry()
    ph = bomb(300, 12, wavelength=350.0)
    ids, rows, final, _ = oracle_steps(oracle_mod, pack_geometry(geo), ph, seed=2, max_steps=8)
    tracks = PhotonTracks.from_steps(ids, rows, len(ph))
    assert len(tracks) == 300 and int(tracks.offsets[-1]) == sum(len(i) for i in ids)
    steps_taken = tracks.steps_taken
    assert steps_taken.min() >= 1 and steps_taken.max() <= 8 and len(np.unique(steps_taken)) > 3
    for i, tr in enumerate(tracks):
        assert_bit_exact(tr[0:1], ph[i:i + 1], 'row 0 of photon %d' % i)
        assert_bit_exact(tr[len(tr) - 1:], final[i:i + 1], 'last row of photon %d' % i)
        assert (np.diff(tr.t) >= 0).all(), 'time runs backwards along track %d' % i
        terminal = (tr.flags & event.TERMINAL_MASK) != 0
        assert not terminal[:-1].any(), 'photon %d goes on after a terminal row' % i
        # a photon stops either because it ended or because the steps ran out
        assert terminal[-1] or steps_taken[i] == 8
        assert steps_taken[i] == len(tr) - 1
