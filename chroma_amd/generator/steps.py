"""Photons from the step points of charged particles: the light source, the segments, and the host generator.

A track's ``event.Steps`` (as a stepping action records them: point 0 the pre-step point with zero deposit, point k + 1
the post-step point of step k with that step's deposits) is cut into SEGMENTS, two consecutive points A -> B of one vertex.
A segment emits Cherenkov light (Frank-Tamm over the wavelength grid) and scintillation light (``light_yield * qedep``) in ONE
medium -- a stepping action limits every step at a volume boundary -- described by a :class:`LightSource`: the same one for
every segment of a call, or, with a :class:`LightMedia` and a ``medium`` array, row ``medium[s]`` of a table of them for
segment s.  ``generate_photons`` here runs the library's host loops (``chroma_steps_count_host`` /
``chroma_steps_generate_host`` and their ``_media_host`` twins): no GPU is needed, and the photons are bit for bit those
``chroma_amd.gpu.steps.generate_photons`` makes on the device from the same segments, seed and ``segment_base``.

Of a Material's scintillation properties ``scintillation_spectrum``, ``scintillation_light_yield`` and
``scintillation_waveform`` are read.  ``scintillation_rise_time`` and ``scintillation_mod`` are NOT: the delay comes from the
waveform alone, and ``qedep`` is taken as it is -- it is already quenched.  No secondary particle is made.  Which medium a
segment lies in is the caller's to say here (``medium``); ``chroma_amd.gpu.steps`` can find it in the geometry itself.
"""
import ctypes

import numpy as np

from chroma_amd import _lib, event
from chroma_amd.geometry import standard_wavelengths

# pdgcode -> (mass in MeV, charge in e): e, mu, pi, K, p and alpha, both signs (PDG 2022 masses)
PARTICLES = {}
for _code, _mass, _z in ((11, 0.51099895, -1), (13, 105.6583755, -1), (211, 139.57039, 1), (321, 493.677, 1),
                         (2212, 938.27208816, 1), (1000020040, 3727.3794066, 2)):
    PARTICLES[_code] = (_mass, float(_z))
    PARTICLES[-_code] = (_mass, float(-_z))


def _uniform_grid(values, what):
    values = np.asarray(values, dtype=np.float64)
    d = np.diff(values)
    if len(values) < 2 or not np.allclose(d, d[0], rtol=1e-6, atol=0) or d[0] <= 0:
        raise ValueError('%s must be rising and equally spaced apart.' % what)
    return float(values[0]), float(d[0])


def _cdf(density, what):
    """The CDF at the nodes of a uniform grid of the density given at them (trapezoids), 0 at the first and 1 at the last."""
    density = np.asarray(density, dtype=np.float64)
    if (density < 0).any() or not np.isfinite(density).all():
        raise ValueError('%s must be finite and not negative' % what)
    c = np.concatenate(([0.0], np.cumsum(0.5 * (density[1:] + density[:-1]))))
    if not c[-1] > 0:
        raise ValueError('%s is zero everywhere on the grid' % what)
    c = (c / c[-1]).astype(np.float32)
    c[-1] = 1.0
    return c


class LightSource(object):
    """One medium as a light source, resampled to the geometry's grids (``wavelengths``, ``times``: what the GPUGeometry
    was made with; the defaults are its defaults).  ``cherenkov_range`` (nm) is snapped to grid nodes: ``wl_lo``, ``wl_hi``.
    A material without ``scintillation_spectrum`` or ``scintillation_light_yield`` gives Cherenkov light only; without
    ``scintillation_waveform`` its scintillation is prompt."""

    def __init__(self, material, wavelengths=None, cherenkov_range=(200, 800), times=None):
        from chroma_amd.gpu.geometry import interp_material_property      # (NumPy only: the resampling the geometry's tables get)
        wl = np.asarray(standard_wavelengths if wavelengths is None else wavelengths, dtype=np.float64)
        if times is None:
            times = np.arange(0, 1000, 0.05)
        if material is None or material.refractive_index is None:
            raise ValueError('a light source needs a material with a refractive index')
        self.material = material
        self.wavelengths = wl
        self.refractive_index = interp_material_property(wl, material.refractive_index)
        lo, hi = (int(np.argmin(np.abs(wl - x))) for x in cherenkov_range)
        if not lo < hi:
            raise ValueError('cherenkov_range must cover at least two grid nodes')
        self.cherenkov_nodes = (lo, hi)
        self.wl_lo, self.wl_hi = float(wl[lo]), float(wl[hi])
        self.light_yield = 0.0
        self.scintillation_cdf = self.time_cdf = None
        if material.scintillation_spectrum is not None and material.scintillation_light_yield:
            self.light_yield = float(material.scintillation_light_yield)
            self.scintillation_cdf = _cdf(interp_material_property(wl, material.scintillation_spectrum), 'scintillation_spectrum')
            if material.scintillation_waveform is not None:
                self.time_cdf = _cdf(interp_material_property(times, material.scintillation_waveform), 'scintillation_waveform')
        s = self.struct = _lib.LightSource()
        s.refractive_index = _lib.ptr(self.refractive_index)
        s.scintillation_cdf = _lib.ptr(self.scintillation_cdf)
        s.time_cdf = _lib.ptr(self.time_cdf)
        s.wavelength_n = len(wl)
        s.wavelength_start, s.wavelength_step = _uniform_grid(wl, 'wavelengths')
        s.time_n = len(times)
        s.time_start, s.time_step = _uniform_grid(times, 'times')
        s.light_yield = self.light_yield
        s.cherenkov_lo, s.cherenkov_hi = lo, hi

    def expected_photons(self, segments):
        """About how many photons ``segments`` emit in all (float64 NumPy, the formulas of the kernels): what a caller
        sizes batches by before anything is drawn."""
        if len(segments) == 0:
            return 0.0
        return float(self.expected_per_segment(segments).sum())

    def expected_per_segment(self, segments):
        """... and segment by segment: float64 (n,)."""
        lo, hi = self.cherenkov_nodes
        wl, n = self.wavelengths[lo:hi + 1], self.refractive_index[lo:hi + 1].astype(np.float64)
        beta2 = np.maximum(segments.beta.astype(np.float64), 1e-30)[:, None] ** 2
        f = np.maximum(0.0, 1.0 - 1.0 / (beta2 * n * n)) / (wl * wl)
        integral = (0.5 * (f[:, 1:] + f[:, :-1]) * np.diff(wl)).sum(axis=1)
        length = np.linalg.norm(segments.b.astype(np.float64) - segments.a, axis=1)
        cherenkov = 2 * np.pi * 7.2973525693e-3 * 1e6 * segments.z.astype(np.float64) ** 2 * length * integral
        return cherenkov + self.light_yield * np.maximum(segments.qedep, 0).astype(np.float64)


class LightMedia(object):
    """Several media as ONE table of light sources, a row per material: ``sources[m]`` is the :class:`LightSource` of
    ``materials[m]``, and ``desc`` the chroma_light_media_desc over their stacked tables (all on the same grids, with the same
    Cherenkov range).  A segment in row m emits exactly what ``sources[m]`` emits for it."""

    def __init__(self, materials, wavelengths=None, cherenkov_range=(200, 800), times=None):
        self.materials = list(materials)
        if not self.materials:
            raise ValueError('light media: no material')
        self.sources = [LightSource(m, wavelengths, cherenkov_range, times) for m in self.materials]
        first = self.sources[0].struct
        nwl, nt = first.wavelength_n, first.time_n
        self.refractive_index = np.ascontiguousarray([s.refractive_index for s in self.sources], dtype=np.float32)
        self.light_yield = np.array([s.light_yield for s in self.sources], dtype=np.float32)
        self.prompt = np.array([s.time_cdf is None for s in self.sources], dtype=np.uint8)
        self.scintillation_cdf = self.time_cdf = None
        if self.light_yield.any():
            self.scintillation_cdf = np.zeros((len(self.sources), nwl), dtype=np.float32)
            for row, s in zip(self.scintillation_cdf, self.sources):
                if s.scintillation_cdf is not None:
                    row[:] = s.scintillation_cdf
        if not self.prompt.all():
            self.time_cdf = np.zeros((len(self.sources), nt), dtype=np.float32)
            for row, s in zip(self.time_cdf, self.sources):
                if s.time_cdf is not None:
                    row[:] = s.time_cdf
        d = self.desc = _lib.LightMediaDesc()
        d.nmedia = len(self.sources)
        for name in ('refractive_index', 'scintillation_cdf', 'time_cdf', 'light_yield', 'prompt'):
            setattr(d, name, _lib.ptr(getattr(self, name)))
        for name in ('wavelength_n', 'wavelength_start', 'wavelength_step', 'time_n', 'time_start', 'time_step', 'cherenkov_lo', 'cherenkov_hi'):
            setattr(d, name, getattr(first, name))

    @classmethod
    def from_geometry(cls, geometry, **kwargs):
        """A row per material of ``geometry.unique_materials``, in that order: row m is the geometry's material index m,
        which is what ``chroma_amd.gpu.steps.locate_materials`` answers with."""
        return cls(geometry.unique_materials, **kwargs)

    def __len__(self):
        return len(self.sources)

    def index(self, material):
        """The row of ``material`` (by identity), or -1."""
        for m, have in enumerate(self.materials):
            if have is material:
                return m
        return -1

    def expected_per_segment(self, segments):
        """(nmedia, n) float64: what each segment is expected to emit in each medium."""
        return np.array([s.expected_per_segment(segments) for s in self.sources]).reshape(len(self.sources), len(segments))

    def expected_photons(self, segments, medium):
        """About how many photons ``segments`` emit in all with segment s in row ``medium[s]`` (rows outside the table: none)."""
        medium = np.asarray(medium, dtype=np.int64)
        if len(segments) == 0:
            return 0.0
        ok = (medium >= 0) & (medium < len(self.sources))
        per = self.expected_per_segment(segments)
        return float(per[np.where(ok, medium, 0), np.arange(len(segments))][ok].sum())

    def expected_at_most(self, segments):
        """An upper bound of ``expected_photons`` that needs no medium array: every segment in the medium it would emit most in."""
        if len(segments) == 0:
            return 0.0
        return float(self.expected_per_segment(segments).max(axis=0).sum())


_SEGMENT_FIELDS = ('a', 'b', 't_a', 't_b', 'beta', 'z', 'qedep', 'evidx')


class Segments(object):
    """Segments as parallel NumPy arrays: ``a``, ``b`` float32 (n, 3) mm; ``t_a``, ``t_b`` ns, ``beta`` (mean of the two
    points'), ``z`` (charge in e; 0: no Cherenkov light), ``qedep`` float32 (n,); ``evidx`` uint32 (n,).  ``segment_base``:
    the global index of segment 0, which keys the random streams -- give the parts of one set of segments consecutive
    bases and they emit the photons the whole set emits."""

    def __init__(self, a, b, t_a, t_b, beta, z, qedep, evidx, segment_base=0):
        self.a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 3)
        self.b = np.ascontiguousarray(b, dtype=np.float32).reshape(-1, 3)
        n = len(self.a)
        for name, v, dtype in (('t_a', t_a, np.float32), ('t_b', t_b, np.float32), ('beta', beta, np.float32), ('z', z, np.float32),
                               ('qedep', qedep, np.float32), ('evidx', evidx, np.uint32)):
            v = np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=dtype), (n,)))
            setattr(self, name, v)
        if len(self.b) != n:
            raise ValueError('segments: arrays of different lengths')
        self.segment_base = int(segment_base)

    def __len__(self):
        return len(self.a)

    def __getitem__(self, key):
        if not isinstance(key, slice) or key.step not in (None, 1):
            raise TypeError('Segments supports contiguous slices only')
        lo = key.indices(len(self))[0]
        return Segments(*[getattr(self, name)[key] for name in _SEGMENT_FIELDS], segment_base=self.segment_base + lo)

    @staticmethod
    def join(parts, segment_base=0):
        parts = list(parts)
        if not parts:
            return Segments(np.zeros((0, 3)), np.zeros((0, 3)), [], [], [], [], [], [], segment_base)
        return Segments(*[np.concatenate([getattr(p, name) for p in parts]) for name in _SEGMENT_FIELDS], segment_base=segment_base)

    def struct(self, pointers=None):
        """chroma_step_segments over these host arrays, or over ``pointers`` (name -> device pointer)."""
        s = _lib.StepSegments()
        for name in _SEGMENT_FIELDS:
            setattr(s, name, pointers[name] if pointers is not None else _lib.ptr(getattr(self, name)))
        s.n = len(self)
        s.segment_base = self.segment_base
        return s


def segments_from_vertices(vertices, evidx=0, segment_base=0):
    """The segments of ``vertices`` (one ``event.Vertex`` or several; those without ``steps`` have none), in vertex order;
    no segment joins two vertices.  ``evidx``: one event index for all, or one per vertex.  Mass and charge come from the
    vertex's ``pdgcode`` (``PARTICLES``); an unknown or neutral particle gets z = 0 and beta = 0: no Cherenkov light."""
    if isinstance(vertices, event.Vertex):
        vertices = [vertices]
    vertices = list(vertices)
    evidx = np.broadcast_to(np.asarray(evidx, dtype=np.uint32), (len(vertices),))
    parts = []
    for v, ev in zip(vertices, evidx):
        st = v.steps
        if st is None or len(np.atleast_1d(st.x)) < 2:
            continue
        p = np.column_stack([np.asarray(st.x, dtype=np.float64), np.asarray(st.y, dtype=np.float64), np.asarray(st.z, dtype=np.float64)])
        t, ke, qedep = (np.asarray(x, dtype=np.float64) for x in (st.t, st.ke, st.qedep))
        mass, z = PARTICLES.get(v.pdgcode, (None, 0.0))
        if mass is None or z == 0.0:
            beta, z = np.zeros(len(t)), 0.0
        else:
            gamma = 1.0 + np.maximum(ke, 0.0) / mass
            beta = np.sqrt(1.0 - 1.0 / (gamma * gamma))
        parts.append(Segments(p[:-1], p[1:], t[:-1], t[1:], 0.5 * (beta[:-1] + beta[1:]), z, qedep[1:], ev))
    return Segments.join(parts, segment_base)


def _as_segments(vertices_or_segments, evidx, segment_base):
    if isinstance(vertices_or_segments, Segments):
        return vertices_or_segments
    return segments_from_vertices(vertices_or_segments, evidx=evidx, segment_base=segment_base)


def _medium_array(segments, source, medium):
    """The int32 row per segment for a LightMedia ``source``; None for a LightSource (which takes no ``medium``)."""
    if not isinstance(source, LightMedia):
        if medium is not None:
            raise ValueError('medium= goes with a LightMedia, not with one LightSource')
        return None
    if medium is None:
        raise ValueError('a LightMedia needs medium=: the row of every segment')
    medium = np.ascontiguousarray(np.broadcast_to(np.asarray(medium, dtype=np.int32), (len(segments),)))
    return medium


def count_photons(segments, source, seed, medium=None):
    """(offsets, total) of the host count: ``offsets`` uint32 (2 n + 1,), the photons of segment s are
    ``offsets[2 s] .. offsets[2 s + 2]``, Cherenkov before scintillation.  ``source``: a LightSource, or a LightMedia with
    ``medium`` (int array, the row of each segment; a row outside the table emits nothing)."""
    offsets = np.zeros(2 * len(segments) + 1, dtype=np.uint32)
    total = ctypes.c_uint64()
    seg = segments.struct()
    seed = int(seed) & (2 ** 64 - 1)
    medium = _medium_array(segments, source, medium)
    if medium is None:
        _lib.check(_lib.load().chroma_steps_count_host(ctypes.byref(source.struct), ctypes.byref(seg), seed, _lib.ptr(offsets), ctypes.byref(total)))
    else:
        _lib.check(_lib.load().chroma_steps_count_media_host(ctypes.byref(source.desc), ctypes.byref(seg), _lib.ptr(medium), seed,
                                                             _lib.ptr(offsets), ctypes.byref(total)))
    return offsets, total.value


def generate_photons(vertices_or_segments, source, seed, evidx=0, segment_base=0, medium=None):
    """The photons ``source`` emits along the segments (or the steps of the vertices), made on the HOST: an
    ``event.Photons`` in segment order, a segment's Cherenkov photons before its scintillation photons.  ``source`` and
    ``medium`` as for ``count_photons``."""
    segments = _as_segments(vertices_or_segments, evidx, segment_base)
    medium = _medium_array(segments, source, medium)
    offsets, n = count_photons(segments, source, seed, medium)
    out = event.Photons(np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros(n, np.float32))
    counters = np.zeros(n, dtype=np.uint32)
    arrays = _lib.PhotonArrays()
    for name in ('pos', 'dir', 'pol', 'wavelengths', 't', 'flags', 'last_hit_triangles', 'weights', 'evidx'):
        setattr(arrays, name, _lib.ptr(getattr(out, name)))
    arrays.rng_counters = _lib.ptr(counters)
    seg = segments.struct()
    seed = int(seed) & (2 ** 64 - 1)
    if medium is None:
        _lib.check(_lib.load().chroma_steps_generate_host(ctypes.byref(source.struct), ctypes.byref(seg), seed, _lib.ptr(offsets),
                                                          ctypes.byref(arrays), n))
    else:
        _lib.check(_lib.load().chroma_steps_generate_media_host(ctypes.byref(source.desc), ctypes.byref(seg), _lib.ptr(medium), seed,
                                                                _lib.ptr(offsets), ctypes.byref(arrays), n))
    return out
