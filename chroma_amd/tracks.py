"""PhotonTracks: the tracks of a set of photons as ONE flat Photons object and the offsets of each photon's rows in it.

A track is what the reference's tracking mode records (chroma/gpu/photon.py:218-238, chroma/sim.py:102-114): row 0 is the
photon before the first step, and every step whose input queue holds the photon adds one row, its state after that step.
``GPUPhotons.propagate_tracks`` fills this layout on the device; ``PhotonTracks.from_steps`` builds the same object from the
per-step lists ``GPUPhotons.propagate(track=True)`` returns.
"""
import numpy as np

from chroma_amd.event import Photons


def host_tracks(step_photon_ids, step_photons, lo, hi):
    """The tracks of the photons ``lo:hi`` of a batch as the reference assembles them on the host (chroma/sim.py:102-114): a list of
    Photons, one per photon, from the per-step lists of ``GPUPhotons.propagate(track=True)``, an append per row.  Like the
    reference's loop it ENDS at the first step none of these photons took part in."""
    tracks = [[] for _ in range(hi - lo)]
    for step_ids, photons in zip(step_photon_ids, step_photons):
        mask = np.logical_and(step_ids >= lo, step_ids < hi)
        if np.count_nonzero(mask) == 0:
            break
        ids = step_ids[mask] - lo
        photons = photons[mask]
        for k, pid in enumerate(ids):
            tracks[pid].append(photons[k])
    return [Photons.join(t, concatenate=False) if len(t) > 0 else Photons() for t in tracks]


class PhotonTracks(object):
    """A sequence of ``Photons``, one per photon: ``tracks[i]`` is rows ``offsets[i]:offsets[i + 1]`` of ``photons``, in step
    order.  ``len``, indexing (negative indices too), slicing and iteration all slice the flat arrays: no per-photon object
    exists until it is asked for.

    ``offsets``: uint64 array of nphotons + 1 entries; ``photons``: the flat rows, an ``event.Photons``."""

    def __init__(self, offsets, photons):
        self.offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        if self.offsets.ndim != 1 or len(self.offsets) < 1:
            raise ValueError('offsets: one entry per photon and one behind the last')
        if int(self.offsets[-1]) != len(photons) or int(self.offsets[0]) != 0:
            raise ValueError('offsets run from %d to %d for %d rows' % (self.offsets[0], self.offsets[-1], len(photons)))
        self.photons = photons
        self._bounds = self.offsets.astype(np.int64)      # (what slices are made of)

    def __len__(self):
        return len(self.offsets) - 1

    @property
    def steps_taken(self):
        """Steps each photon took part in: its rows but the first."""
        return np.diff(self._bounds) - 1

    def cut(self, lo, hi):
        """The tracks of photons ``lo:hi`` as a PhotonTracks of their own (views of the flat arrays)."""
        b = self._bounds[lo:hi + 1]
        return PhotonTracks((b - b[0]).astype(np.uint64), self.photons[int(b[0]):int(b[-1])])

    def __getitem__(self, key):
        n = len(self)
        if isinstance(key, slice):
            start, stop, step = key.indices(n)
            if step == 1:
                return self.cut(start, max(start, stop))
            return [self[i] for i in range(start, stop, step)]
        i = int(key)
        if i < 0:
            i += n
        if not 0 <= i < n:
            raise IndexError('photon %d of %d' % (key, n))
        return self.photons[int(self._bounds[i]):int(self._bounds[i + 1])]

    def __iter__(self):
        photons, b = self.photons, self._bounds.tolist()
        for lo, hi in zip(b[:-1], b[1:]):
            yield photons[lo:hi]

    @staticmethod
    def from_steps(step_photon_ids, step_photons, nphotons):
        """From the reference-shaped lists of tracking mode: entry k of ``step_photon_ids`` names the photons whose rows
        entry k of ``step_photons`` holds (entry 0: every photon before the first step; entry k: the photons that entered
        step k, as they are after it).  A photon's rows keep the order of the steps."""
        nphotons = int(nphotons)
        parts = [(np.asarray(ids, dtype=np.int64), p) for ids, p in zip(step_photon_ids, step_photons) if len(ids)]
        if not parts:
            return PhotonTracks(np.zeros(nphotons + 1, dtype=np.uint64), Photons())
        ids = np.concatenate([i for i, _ in parts])
        rows = Photons.join([p for _, p in parts])
        if len(rows) != len(ids):
            raise ValueError('%d photon ids for %d rows' % (len(ids), len(rows)))
        if len(ids) and (ids.min() < 0 or ids.max() >= nphotons):
            raise ValueError('photon id outside 0..%d' % nphotons)
        # (the lists are in step order already: a stable sort by photon keeps it within each photon)
        order = np.argsort(ids, kind='stable')
        offsets = np.concatenate(([0], np.cumsum(np.bincount(ids, minlength=nphotons)))).astype(np.uint64)
        return PhotonTracks(offsets, rows[order])
