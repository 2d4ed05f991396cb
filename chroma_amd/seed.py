"""A seed for an event's vertex: the position and time at which the hits' time residuals pile up best (the definition is in
include/chroma_hip.h, "vertex seed").  ``VertexSeeder`` turns channel positions, a speed of light and (channel, time, weight)
rows into the integers of chroma_vertex_seed_host / chroma_vertex_seed and the integers that come back into mm and ns.  It is a
SEED: one straight-line speed, no scattering, no direction -- what a likelihood starts from, not what it ends at.  No GPU is
needed here; ``chroma_amd.gpu.seed.GPUVertexSeeder`` runs the same fits on the device.

``DirectionSeeder`` adds the direction about such a vertex ("direction seed" in the same header: a cone fit, chroma_direction_seed_host
/ chroma_direction_seed, ``chroma_amd.gpu.seed.GPUDirectionSeeder``), and ``to_vertices`` makes ``event.Vertex`` of the two."""
import ctypes
import math

import numpy as np

from chroma_amd import _lib

MAX_COORD, MAX_BINS, MAX_SHAPE, MAX_LEVELS, MAX_CAND, MAX_FIT_HITS, MAX_STEP = 2 ** 23, 1024, 16, 8, 2 ** 20, 65535, 2 ** 21
MAX_SLOWNESS, MAX_BIN_TICKS = 2 ** 24, 2 ** 20
LAST_TICK = 2 ** 31 - 1


class SeedFits(object):
    """The fits of one ``fit_many``: ``pos`` (n x 3 float64, mm), ``t0`` (ns, float64: the lower edge of the residual bin under
    the shape's first maximum), ``score``, ``bin``, ``cand`` (the level-0 candidate), ``outside`` (hits that fell out of the
    histogram at the final point), ``nhits`` (uint32), ``level_score`` (n x (levels + 1), uint32) and, when asked for, ``scores``
    (n x candidates, uint32); ``pos_int`` (n x 3 int32) are the positions in position units."""

    def __init__(self, pos, t0, score, bin, cand, level_score, outside, nhits, pos_int, scores=None):
        self.pos, self.t0, self.score, self.bin, self.cand, self.level_score = pos, t0, score, bin, cand, level_score
        self.outside, self.nhits, self.pos_int, self.scores = outside, nhits, pos_int, scores

    def __len__(self):
        return len(self.score)

    def __getitem__(self, key):
        """The fits ``key`` (a slice) as a ``SeedFits`` of their own."""
        if not isinstance(key, slice):
            raise TypeError('SeedFits takes slices')
        return SeedFits(*[getattr(self, n)[key] for n in ('pos', 't0', 'score', 'bin', 'cand', 'level_score', 'outside', 'nhits', 'pos_int')],
                        scores=None if self.scores is None else self.scores[key])


class PreparedFits(object):
    """What one call takes (``VertexSeeder.prepare``): the ``_lib.VertexSeeder`` struct, ``offsets`` (uint32), ``tau0`` (int32),
    the hit arrays (int32, int32, uint32) and ``origin`` (int64 per fit: the tick the fit's times are counted from)."""

    def __init__(self, struct, offsets, tau0, channel, time, weight, origin):
        self.struct, self.offsets, self.tau0, self.channel, self.time, self.weight, self.origin = struct, offsets, tau0, channel, time, weight, origin
        self.nfits = len(offsets) - 1


def _round_half_up(x):
    return np.floor(np.asarray(x, dtype=np.float64) + 0.5)


class VertexSeeder(object):
    """``positions_mm`` (channels x 3), ``speed_mm_per_ns`` the one speed light is taken to travel at; ``bin_ns`` the width of a
    residual bin and ``ticks_per_bin`` its ticks (times are rounded to ticks); ``shape`` up to 16 integers 0 .. 255 (default:
    ``gaussian_shape(bin_ns, bin_ns)``); ``pos_unit_mm`` the position unit; ``candidates_mm`` the level-0 candidates (default: a
    cubic grid of ``spacing_mm``, default radius / 8, inside the sphere about the channels' centroid that reaches the farthest
    channel); ``levels`` refinement levels, the first on a lattice of half the spacing; ``weights``: 'unit' (a hit counts 1) or
    'npe' (its weight, rounded, 255 at the most)."""

    def __init__(self, positions_mm, speed_mm_per_ns, bin_ns=1.0, shape=None, spacing_mm=None, levels=6, pos_unit_mm=0.125, ticks_per_bin=16,
                 candidates_mm=None, weights='unit'):
        positions = np.asarray(positions_mm, dtype=np.float64).reshape(-1, 3)
        if not (speed_mm_per_ns > 0 and bin_ns > 0 and pos_unit_mm > 0):
            raise ValueError('speed, bin and position unit are positive')
        if weights not in ('unit', 'npe'):
            raise ValueError("weights is 'unit' or 'npe'")
        if not 0 <= int(levels) <= MAX_LEVELS:
            raise ValueError('0 .. %d levels' % MAX_LEVELS)
        if not 1 <= int(ticks_per_bin) <= MAX_BIN_TICKS:
            raise ValueError('1 .. 2^20 ticks per bin')
        self.speed, self.bin_ns, self.levels, self.unit, self.bin_ticks, self.weights = float(speed_mm_per_ns), float(bin_ns), int(levels), float(pos_unit_mm), int(ticks_per_bin), weights
        self.tick_ns = self.bin_ns / self.bin_ticks
        self.channel_pos = self._units(positions, 'channel')
        self.nchannels = len(positions)
        slowness = int(_round_half_up(65536.0 * self.unit / (self.speed * self.tick_ns)))
        if not 1 <= slowness <= MAX_SLOWNESS:
            raise ValueError('the speed is %g ticks per position unit in 1/65536: outside 1 .. 2^24, choose another unit or tick' % slowness)
        self.slowness = slowness
        self.shape = np.asarray(self.gaussian_shape(self.bin_ns, self.bin_ns) if shape is None else shape, dtype=np.int64).reshape(-1)
        if not 1 <= len(self.shape) <= MAX_SHAPE or self.shape.min() < 0 or self.shape.max() > 255 or self.shape.max() < 1:
            raise ValueError('the shape has 1 .. 16 entries of 0 .. 255, one of them positive')
        self.centre = positions.mean(axis=0) if len(positions) else np.zeros(3)
        self.radius = float(np.sqrt(((positions - self.centre) ** 2).sum(axis=1)).max()) if len(positions) else 0.0
        self.spacing = float(spacing_mm) if spacing_mm is not None else max(self.radius / 8.0, self.unit)
        if not self.spacing > 0:
            raise ValueError('the spacing is positive')
        candidates = self._grid() if candidates_mm is None else np.asarray(candidates_mm, dtype=np.float64).reshape(-1, 3)
        if not 1 <= len(candidates) <= MAX_CAND:
            raise ValueError('1 .. 2^20 candidates (%d)' % len(candidates))
        self.cand = self._units(candidates, 'candidate')
        self.step = min(MAX_STEP, int(_round_half_up(0.5 * self.spacing / self.unit)))
        # the ticks light takes across the sphere, by the definition's own arithmetic
        self.across = (int(math.ceil(2.0 * self.radius / self.unit)) * self.slowness + 32768) >> 16
        self.peak = int(np.argmax(self.shape))          # (the first maximum)

    @classmethod
    def for_detector(cls, detector, speed_mm_per_ns, **kw):
        """The seeder of ``detector``'s channels (``channel_index_to_position``; a channel without a position is at the origin)."""
        positions = [np.zeros(3) if p is None else np.asarray(p, dtype=np.float64) for p in detector.channel_index_to_position]
        return cls(np.asarray(positions, dtype=np.float64).reshape(-1, 3), speed_mm_per_ns, **kw)

    @classmethod
    def of(cls, value, detector):
        """``value`` if it is a ``VertexSeeder``; else the seeder of ``detector``'s channels for a speed in mm/ns or a (speed[,
        spacing_mm[, levels]])."""
        if isinstance(value, cls):
            return value
        parts = list(value) if isinstance(value, (tuple, list)) else [value]
        if not 1 <= len(parts) <= 3:
            raise ValueError('a seeder: a VertexSeeder, a speed or (speed[, spacing_mm[, levels]])')
        kw = {}
        if len(parts) > 1:
            kw['spacing_mm'] = float(parts[1])
        if len(parts) > 2:
            kw['levels'] = int(parts[2])
        return cls.for_detector(detector, float(parts[0]), **kw)

    @staticmethod
    def gaussian_shape(sigma_ns, bin_ns, tail_ns=0.0):
        """Up to 16 integers 0 .. 255: a Gaussian of ``sigma_ns`` sampled at bin centres about its peak, 255 at the peak, with an
        exponential tail of ``tail_ns`` on the late side where that is higher; entries that round to 0 at the ends are dropped."""
        half = int(min(7, max(0, math.ceil(3.0 * sigma_ns / bin_ns))))
        late = 8 if tail_ns > 0 else half
        values = []
        for j in range(-half, late + 1):
            x = j * bin_ns
            v = math.exp(-0.5 * (x / sigma_ns) ** 2) if sigma_ns > 0 else float(j == 0)
            if j > 0 and tail_ns > 0:
                v = max(v, math.exp(-x / tail_ns))
            values.append(int(math.floor(255.0 * v + 0.5)))
        while values[0] == 0:
            values.pop(0)
        while values[-1] == 0:
            values.pop()
        return values[:MAX_SHAPE]

    def _units(self, mm, what):
        u = _round_half_up(np.asarray(mm, dtype=np.float64) / self.unit)
        if not np.all(np.abs(u) <= MAX_COORD):          # (a NaN fails too)
            raise ValueError('a %s lies beyond 2^23 position units of %g mm' % (what, self.unit))
        return np.ascontiguousarray(u.astype(np.int32).reshape(-1, 3))

    def _grid(self):
        n = int(math.floor(self.radius / self.spacing))
        axis = np.arange(-n, n + 1, dtype=np.float64) * self.spacing
        k, j, i = np.meshgrid(axis, axis, axis, indexing='ij')          # (x runs fastest)
        offsets = np.stack([i.ravel(), j.ravel(), k.ravel()], axis=1)
        return self.centre + offsets[(offsets ** 2).sum(axis=1) <= self.radius ** 2 * (1.0 + 1e-12)]

    def struct(self, nbins):
        s = _lib.VertexSeeder(self.slowness, self.bin_ticks, int(nbins), len(self.shape), self.step, self.levels)
        for j, v in enumerate(self.shape):
            s.shape[j] = int(v)
        return s

    def prepare(self, offsets, channel, t_ns, weight=None):
        """The integers of one call.  Per fit: ticks = floor(t / tick + 0.5) counted from the fit's earliest tick (a hit later than
        2^31 - 1 ticks after it is taken there); tau0 = minus the ticks light takes across the sphere.  The call's bins cover the
        longest fit's span plus that crossing, 1024 at the most: later hits fall OUTSIDE and are counted there."""
        offsets = np.asarray(offsets, dtype=np.int64).reshape(-1)
        if len(offsets) < 1 or offsets[0] != 0 or np.any(np.diff(offsets) < 0):
            raise ValueError('offsets start at 0 and do not descend')
        nfits, nhits = len(offsets) - 1, int(offsets[-1])
        channel = np.ascontiguousarray(np.asarray(channel).reshape(-1), dtype=np.int32)
        t = np.asarray(t_ns, dtype=np.float64).reshape(-1)
        if len(channel) != nhits or len(t) != nhits:
            raise ValueError('%d hits by the offsets, %d channels and %d times' % (nhits, len(channel), len(t)))
        if np.any(np.diff(offsets) > MAX_FIT_HITS):
            raise ValueError('a fit holds %d hits at the most' % MAX_FIT_HITS)
        if not np.all(np.isfinite(t)):
            raise ValueError('a hit time is not finite')
        if self.weights == 'unit' or weight is None:
            w = np.ones(nhits, dtype=np.uint32)
        else:
            w = np.clip(_round_half_up(np.asarray(weight, dtype=np.float64).reshape(-1)), 0, 2 ** 32 - 1).astype(np.uint32)
            if len(w) != nhits:
                raise ValueError('%d hits, %d weights' % (nhits, len(w)))
        ticks = _round_half_up(t / self.tick_ns)
        origin = np.zeros(nfits, dtype=np.int64)
        has = np.diff(offsets) > 0
        span = 0
        if nhits:
            starts = offsets[:-1][has]
            first = np.minimum.reduceat(ticks, starts)
            if not np.all(np.abs(first) < 2.0 ** 62):
                raise ValueError('a hit time is beyond 2^62 ticks')
            origin[has] = first.astype(np.int64)
            rel = np.minimum(ticks - np.repeat(first, np.diff(offsets)[has]), float(LAST_TICK))
            span = int(rel.max())
        else:
            rel = np.zeros(0)
        nbins = max(1, min(MAX_BINS, -(-(span + self.across + 1) // self.bin_ticks)))
        tau0 = np.full(nfits, -self.across, dtype=np.int64)
        if self.across > 2 ** 31 - 1:
            raise ValueError('light takes more than 2^31 ticks across the detector: choose a longer tick')
        return PreparedFits(self.struct(nbins), np.ascontiguousarray(offsets, dtype=np.uint32), np.ascontiguousarray(tau0, dtype=np.int32), channel,
                            np.ascontiguousarray(rel, dtype=np.int32), np.ascontiguousarray(w), origin)

    def run_host(self, prepared, scores=False):
        """chroma_vertex_seed_host on ``prepared``: (best_pos, best_score, best_bin, best_cand, outside, level_score, scores or None)."""
        lib = _lib.load()
        n = prepared.nfits
        out = self.outputs(n, scores)
        _lib.check(lib.chroma_vertex_seed_host(ctypes.byref(prepared.struct), self.nchannels, _lib.ptr(self.channel_pos), len(self.cand), _lib.ptr(self.cand), n,
                                               _lib.ptr(prepared.offsets), _lib.ptr(prepared.tau0), _lib.ptr(prepared.channel), _lib.ptr(prepared.time),
                                               _lib.ptr(prepared.weight), *[_lib.ptr(a) for a in out]))
        return out

    def outputs(self, nfits, scores):
        """zeroed host arrays in the order of the calls' output arguments"""
        return [np.zeros((nfits, 3), dtype=np.int32)] + [np.zeros(nfits, dtype=np.uint32) for _ in range(4)] + \
               [np.zeros((nfits, self.levels + 1), dtype=np.uint32), np.zeros((nfits, len(self.cand)), dtype=np.uint32) if scores else None]

    def finish(self, prepared, out):
        """The ``SeedFits`` of a call's output arrays."""
        best_pos, best_score, best_bin, best_cand, outside, level_score, scores = out
        ticks = prepared.origin + prepared.tau0.astype(np.int64) + (best_bin.astype(np.int64) + self.peak) * self.bin_ticks
        return SeedFits(best_pos.astype(np.float64) * self.unit, ticks.astype(np.float64) * self.tick_ns, best_score, best_bin, best_cand, level_score, outside,
                        np.diff(prepared.offsets.astype(np.int64)).astype(np.uint32), best_pos, scores)

    def fit_many(self, offsets, channel, t_ns, weight=None, gpu=None, scores=False):
        """The ``SeedFits`` of the fits [offsets[f], offsets[f + 1]) of the hit rows, in ONE call: on the host (``gpu`` None:
        chroma_vertex_seed_host) or on the device (``gpu``: a ``chroma_amd.gpu.seed.GPUVertexSeeder`` of this seeder, or a
        context to make one on) -- the same bits."""
        prepared = self.prepare(offsets, channel, t_ns, weight)
        if gpu is None:
            return self.finish(prepared, self.run_host(prepared, scores))
        from chroma_amd.gpu.seed import GPUVertexSeeder
        runner = gpu if isinstance(gpu, GPUVertexSeeder) else GPUVertexSeeder(gpu, self)
        if runner.seeder is not self:
            raise ValueError('the GPUVertexSeeder was made for another seeder')
        return self.finish(prepared, runner.run(prepared, scores))

    def fit(self, channel, t_ns, weight=None, gpu=None, scores=False):
        """``fit_many`` of one fit."""
        return self.fit_many([0, len(np.asarray(channel).reshape(-1))], channel, t_ns, weight, gpu=gpu, scores=scores)


# ---- the direction seed (include/chroma_hip.h, "direction seed") ----
ONE, MAX_COMPONENT, MAX_DIR_STEP, MAX_FIRST, MAX_WIDTH = 2 ** 14, 2 ** 15, 2 ** 13, 1040, 2048


class DirFits(object):
    """The fits of one ``DirectionSeeder.fit_many``: ``dir`` (n x 3 float64 unit vectors; zeros where the fit has none), ``dir_int``
    (n x 3 int32, Q14), ``score``, ``cand`` (the level-0 candidate), ``level_score`` (n x (levels + 1)), ``inside`` (the summed
    weight of the hits that took part: an energy proxy), ``outside`` (hits that did not), ``nhits`` (uint32) and, when asked for,
    ``cos_hist`` (n x 2^log2_ncos, uint32: the weight per bin of the cosine to ``dir``)."""

    NAMES = ('dir', 'dir_int', 'score', 'cand', 'level_score', 'inside', 'outside', 'nhits')

    def __init__(self, dir, dir_int, score, cand, level_score, inside, outside, nhits, cos_hist=None):
        self.dir, self.dir_int, self.score, self.cand, self.level_score = dir, dir_int, score, cand, level_score
        self.inside, self.outside, self.nhits, self.cos_hist = inside, outside, nhits, cos_hist

    def __len__(self):
        return len(self.score)

    def __getitem__(self, key):
        """The fits ``key`` (a slice) as a ``DirFits`` of their own."""
        if not isinstance(key, slice):
            raise TypeError('DirFits takes slices')
        return DirFits(*[getattr(self, n)[key] for n in self.NAMES], cos_hist=None if self.cos_hist is None else self.cos_hist[key])


class PreparedDirFits(object):
    """What one call takes (``DirectionSeeder.prepare``): the ``_lib.DirectionSeeder`` struct, ``timing`` (the vertex seeder's struct of
    the same rows), ``offsets``, ``tau0``, ``vertex`` (int32, fits x 3), ``bin`` (uint32) and the hit arrays; ``time`` is None
    where no prompt cut is made."""

    def __init__(self, struct, timing, offsets, tau0, vertex, bin, channel, time, weight):
        self.struct, self.timing, self.offsets, self.tau0, self.vertex, self.bin = struct, timing, offsets, tau0, vertex, bin
        self.channel, self.time, self.weight = channel, time, weight
        self.nfits = len(offsets) - 1


class DirectionSeeder(object):
    """The direction a ``VertexSeeder``'s fits lack: ``vertex_seeder`` lends its units, timing, weights and channel positions;
    ``profile`` up to 2^``log2_ncos`` integers 0 .. 255 over the cosine between a hit (seen from the vertex) and the direction, bin k
    covering [k, k + 1) * 2 / 2^log2_ncos - 1 (default: ``cherenkov_profile(0.75, 0.1)``); ``directions`` the level-0 candidates (default:
    a cube-sphere grid of 6 * ``grid``^2); ``levels`` refinement levels, the first on a lattice of half the grid's angular spacing;
    ``prompt_ns``: None -- every hit with a channel takes part -- or (before, after): only hits whose time residual about the
    vertex lies within that window about the seed's t0."""

    def __init__(self, vertex_seeder, profile=None, log2_ncos=6, directions=None, grid=12, levels=6, prompt_ns=None):
        if not 4 <= int(log2_ncos) <= 8:
            raise ValueError('log2_ncos is 4 .. 8')
        if not 0 <= int(levels) <= MAX_LEVELS:
            raise ValueError('0 .. %d levels' % MAX_LEVELS)
        if not int(grid) >= 1:
            raise ValueError('the grid has 1 cell a face edge at the least')
        self.vertex_seeder, self.log2_ncos, self.levels, self.grid = vertex_seeder, int(log2_ncos), int(levels), int(grid)
        profile = self.cherenkov_profile(0.75, 0.1, log2_ncos=self.log2_ncos) if profile is None else profile
        self.profile = np.asarray(profile, dtype=np.int64).reshape(-1)
        if len(self.profile) != 2 ** self.log2_ncos or self.profile.min() < 0 or self.profile.max() > 255 or self.profile.max() < 1:
            raise ValueError('the profile has 2^log2_ncos entries of 0 .. 255, one of them positive')
        if directions is None:
            directions = self.cube_sphere(self.grid)
            spacing = 0.5 * math.pi / self.grid
        else:
            directions = np.asarray(directions, dtype=np.float64).reshape(-1, 3)
            spacing = math.sqrt(4.0 * math.pi / max(1, len(directions)))
        if not 1 <= len(directions) <= MAX_CAND:
            raise ValueError('1 .. 2^20 candidate directions (%d)' % len(directions))
        cand = _round_half_up(ONE * np.asarray(directions, dtype=np.float64))
        if not np.all(np.abs(cand) <= MAX_COMPONENT):
            raise ValueError('a candidate direction is longer than 2')
        self.cand = np.ascontiguousarray(cand.astype(np.int32).reshape(-1, 3))
        self.step = min(MAX_DIR_STEP, int(_round_half_up(0.5 * spacing * ONE)))
        self.first, self.width = 0, 1
        self.prompt = None
        if prompt_ns is not None:
            before, after = float(prompt_ns[0]), float(prompt_ns[1])
            if not (before >= 0 and after >= 0):
                raise ValueError('prompt_ns is (before, after), neither negative')
            # bins about the one under the shape's first maximum, which lies `peak` bins behind the seed's bin
            lo = vertex_seeder.peak - int(math.ceil(before / vertex_seeder.bin_ns))
            hi = vertex_seeder.peak + int(math.ceil(after / vertex_seeder.bin_ns))
            self.first = min(MAX_FIRST, max(0, lo))
            self.width = min(MAX_WIDTH, max(1, hi - self.first + 1))
            self.prompt = (before, after)

    @staticmethod
    def cube_sphere(grid):
        """6 * grid^2 unit vectors: the centres of an equal-angle grid on each face of the cube, face by face (+x, -x, +y, -y, +z, -z)."""
        a = (np.arange(grid) + 0.5) / grid * (0.5 * math.pi) - 0.25 * math.pi
        v, u = np.meshgrid(np.tan(a), np.tan(a), indexing='ij')          # (u runs fastest)
        u, v, one = u.ravel(), v.ravel(), np.ones(grid * grid)
        faces = [(one, u, v), (-one, u, v), (u, one, v), (u, -one, v), (u, v, one), (u, v, -one)]
        d = np.concatenate([np.stack(f, axis=1) for f in faces])
        return d / np.sqrt((d ** 2).sum(axis=1))[:, None]

    @staticmethod
    def cherenkov_profile(cos_c, sigma_cos, fill=0.0, log2_ncos=6):
        """2^log2_ncos integers 0 .. 255: a Gaussian of ``sigma_cos`` about ``cos_c`` sampled at the bins' centres, 255 at its
        highest entry, and ``fill`` (0 .. 1 of that) at the least inside the cone, in the bins centred above ``cos_c``."""
        n = 2 ** int(log2_ncos)
        centres = [(k + 0.5) * 2.0 / n - 1.0 for k in range(n)]
        values = [math.exp(-0.5 * ((c - cos_c) / sigma_cos) ** 2) if sigma_cos > 0 else 0.0 for c in centres]
        top = max(values)
        if top > 0:
            values = [v / top for v in values]
        else:          # (a width of 0, or a peak out of every centre's reach: the bin that holds cos_c)
            values[min(n - 1, max(0, int(math.floor((cos_c + 1.0) * n / 2.0))))] = 1.0
        values = [max(v, float(fill)) if c > cos_c else v for c, v in zip(centres, values)]
        return [int(math.floor(255.0 * min(v, 1.0) + 0.5)) for v in values]

    @classmethod
    def of(cls, value, vertex_seeder):
        """``value`` if it is a ``DirectionSeeder`` (of ``vertex_seeder``); else the one of ``vertex_seeder`` for a cos_c or a (cos_c[,
        sigma_cos[, fill[, levels]]])."""
        if isinstance(value, cls):
            if value.vertex_seeder is not vertex_seeder:
                raise ValueError('the DirectionSeeder was made for another VertexSeeder')
            return value
        parts = list(value) if isinstance(value, (tuple, list)) else [value]
        if not 1 <= len(parts) <= 4:
            raise ValueError('a direction seeder: a DirectionSeeder, a cos_c or (cos_c[, sigma_cos[, fill[, levels]]])')
        sigma = float(parts[1]) if len(parts) > 1 else 0.1
        fill = float(parts[2]) if len(parts) > 2 else 0.0
        kw = {'levels': int(parts[3])} if len(parts) > 3 else {}
        return cls(vertex_seeder, profile=cls.cherenkov_profile(float(parts[0]), sigma, fill), **kw)

    def struct(self):
        s = _lib.DirectionSeeder(self.log2_ncos, self.step, self.levels, self.first, self.width)
        for k, v in enumerate(self.profile):
            s.profile[k] = int(v)
        return s

    def prepare(self, seed_fits, offsets, channel, t_ns=None, weight=None, prepared=None):
        """The integers of one call about ``seed_fits`` (a ``SeedFits`` of the same rows: its ``pos_int`` and ``bin``).  The rows are
        quantised by the vertex seeder's own ``prepare`` (``prepared``: what it returned for them, if at hand), so ticks, tau0 and
        bins mean what they meant to the vertex seed; without ``prompt_ns`` no times are passed."""
        v = self.vertex_seeder
        if prepared is None:
            n = len(np.asarray(channel).reshape(-1))
            if self.prompt is not None and t_ns is None:
                raise ValueError('a prompt cut needs the hit times')
            prepared = v.prepare(offsets, channel, np.zeros(n) if t_ns is None else t_ns, weight)
        if len(seed_fits) != prepared.nfits:
            raise ValueError('%d fits by the offsets, %d seed fits' % (prepared.nfits, len(seed_fits)))
        timed = self.prompt is not None
        return PreparedDirFits(self.struct(), prepared.struct, prepared.offsets, prepared.tau0, np.ascontiguousarray(seed_fits.pos_int, dtype=np.int32).reshape(-1, 3),
                               np.ascontiguousarray(seed_fits.bin, dtype=np.uint32), prepared.channel, prepared.time if timed else None, prepared.weight)

    def outputs(self, nfits, cos_hist):
        """zeroed host arrays in the order of the calls' output arguments"""
        return [np.zeros((nfits, 3), dtype=np.int32)] + [np.zeros(nfits, dtype=np.uint32) for _ in range(4)] + \
               [np.zeros((nfits, self.levels + 1), dtype=np.uint32), np.zeros((nfits, 2 ** self.log2_ncos), dtype=np.uint32) if cos_hist else None]

    def run_host(self, prepared, cos_hist=False):
        """chroma_direction_seed_host on ``prepared``: (best_dir, best_score, best_cand, inside, outside, level_score, cos_hist or None)."""
        lib = _lib.load()
        v = self.vertex_seeder
        out = self.outputs(prepared.nfits, cos_hist)
        _lib.check(lib.chroma_direction_seed_host(ctypes.byref(prepared.struct), ctypes.byref(prepared.timing), v.nchannels, _lib.ptr(v.channel_pos), len(self.cand),
                                                  _lib.ptr(self.cand), prepared.nfits, _lib.ptr(prepared.offsets), _lib.ptr(prepared.tau0), _lib.ptr(prepared.vertex),
                                                  _lib.ptr(prepared.bin), _lib.ptr(prepared.channel), _lib.ptr(prepared.time), _lib.ptr(prepared.weight),
                                                  *[_lib.ptr(a) for a in out]))
        return out

    def finish(self, prepared, out):
        """The ``DirFits`` of a call's output arrays."""
        best_dir, best_score, best_cand, inside, outside, level_score, cos_hist = out
        length = np.sqrt((best_dir.astype(np.float64) ** 2).sum(axis=1))
        unit = best_dir.astype(np.float64) / np.where(length > 0, length, 1.0)[:, None]
        return DirFits(unit, best_dir, best_score, best_cand, level_score, inside, outside, np.diff(prepared.offsets.astype(np.int64)).astype(np.uint32), cos_hist)

    def fit_many(self, seed_fits, offsets, channel, t_ns=None, weight=None, gpu=None, cos_hist=False):
        """The ``DirFits`` of the fits [offsets[f], offsets[f + 1]) of the hit rows about ``seed_fits``, in ONE call: on the host
        (``gpu`` None: chroma_direction_seed_host) or on the device (``gpu``: a ``chroma_amd.gpu.seed.GPUDirectionSeeder`` of this
        seeder, or a context to make one on) -- the same bits."""
        prepared = self.prepare(seed_fits, offsets, channel, t_ns, weight)
        if gpu is None:
            return self.finish(prepared, self.run_host(prepared, cos_hist))
        from chroma_amd.gpu.seed import GPUDirectionSeeder
        runner = gpu if isinstance(gpu, GPUDirectionSeeder) else GPUDirectionSeeder(gpu, self)
        if runner.seeder is not self:
            raise ValueError('the GPUDirectionSeeder was made for another seeder')
        return self.finish(prepared, runner.run(prepared, cos_hist))

    def fit(self, seed_fits, channel, t_ns=None, weight=None, gpu=None, cos_hist=False):
        """``fit_many`` of one fit."""
        return self.fit_many(seed_fits, [0, len(np.asarray(channel).reshape(-1))], channel, t_ns, weight, gpu=gpu, cos_hist=cos_hist)


def to_vertices(seed_fits, dir_fits, particle_name, ke):
    """The ``event.Vertex`` list a likelihood or the stepper starts from: fit k's seed position (mm) and time (ns), its seeded
    direction, and the caller's particle and kinetic energy (one for all, or one per fit) -- the seeds give no energy."""
    from chroma_amd import event
    if len(seed_fits) != len(dir_fits):
        raise ValueError('%d seed fits, %d direction fits' % (len(seed_fits), len(dir_fits)))
    energies = np.broadcast_to(np.asarray(ke, dtype=np.float64), (len(seed_fits),))
    return [event.Vertex(particle_name, np.array(seed_fits.pos[k], dtype=np.float64), np.array(dir_fits.dir[k], dtype=np.float64), float(energies[k]),
                         t0=float(seed_fits.t0[k])) for k in range(len(seed_fits))]
