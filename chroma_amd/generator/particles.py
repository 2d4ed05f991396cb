"""Charged particles stepped through matter in the continuous-slowing-down approximation (CSDA): what makes the
``event.Steps`` that ``chroma_amd.generator.steps`` turns into Cherenkov and scintillation photons.  No GEANT4.

The model.  A particle loses the MEAN stopping power of the medium it is in, read from a table per medium
and species (:class:`StoppingMedia`), in steps limited by ``max_step``, by the fraction ``max_loss`` of its kinetic energy and
by the next volume boundary; below ``ke_cut`` it deposits the rest and stops.  At the end of a step the direction is
scattered by the Highland formula.  Deliberately left out: secondaries (delta rays, bremsstrahlung photons, showers,
decays), energy-loss straggling, the density effect and shell corrections, lateral displacement, positron-specific (Bhabha)
loss, and neutral particles (a vertex of one gets its vertex point alone, status ``UNTRACKED``).

Units: MeV, mm, ns, g/cm^3.  ``track`` here runs the library's host loop in ONE medium (``chroma_particles_track_host``): no
GPU is needed, and the tracks are bit for bit those ``chroma_amd.gpu.particles.track`` makes on the device without a
geometry.  In a geometry the device loop limits every step at the volume boundaries with the engine's own ray cast.
"""
import copy
import ctypes

import numpy as np

from chroma_amd import _lib, event
from chroma_amd.generator.steps import PARTICLES, Segments

__all__ = ['ELEMENTS', 'SPECIES', 'PDG_CODES', 'StoppingMedia', 'Stepper', 'Tracks', 'track', 'STATUS']

ELECTRON_MASS = 0.51099895          # MeV
K_BETHE = 0.307075                  # MeV cm^2 / mol

# symbol -> (Z, A in g/mol)
ELEMENTS = {
    'H': (1, 1.008), 'He': (2, 4.0026), 'Li': (3, 6.94), 'Be': (4, 9.0122), 'B': (5, 10.81), 'C': (6, 12.011), 'N': (7, 14.007),
    'O': (8, 15.999), 'F': (9, 18.998), 'Ne': (10, 20.180), 'Na': (11, 22.990), 'Mg': (12, 24.305), 'Al': (13, 26.982),
    'Si': (14, 28.085), 'P': (15, 30.974), 'S': (16, 32.06), 'Cl': (17, 35.45), 'Ar': (18, 39.948), 'K': (19, 39.098),
    'Ca': (20, 40.078), 'Ti': (22, 47.867), 'Fe': (26, 55.845), 'Ni': (28, 58.693), 'Cu': (29, 63.546), 'Xe': (54, 131.293),
    'Gd': (64, 157.25), 'Pb': (82, 207.2),
}

# |pdg code| -> row of a medium's table: e, mu, pi, K, p, alpha (both signs share a row)
SPECIES = {11: 0, 13: 1, 211: 2, 321: 3, 2212: 4, 1000020040: 5}
SPECIES_MASS = [PARTICLES[code][0] for code in sorted(SPECIES, key=SPECIES.get)]
SPECIES_CHARGE = [abs(PARTICLES[code][1]) for code in sorted(SPECIES, key=SPECIES.get)]

# particle name -> pdg code, for a Vertex whose pdgcode is None
PDG_CODES = {'e-': 11, 'e+': -11, 'mu-': 13, 'mu+': -13, 'pi+': 211, 'pi-': -211, 'K+': 321, 'K-': -321,
             'p': 2212, 'proton': 2212, 'p+': 2212, 'anti_proton': -2212, 'p~': -2212, 'alpha': 1000020040, 'anti_alpha': -1000020040}

STATUS = {'ALIVE': 0, 'STOPPED': 1, 'LEFT': 2, 'TRUNCATED': 3, 'UNTRACKED': 4, 'NAN_ABORT': 5}


def element_excitation_energy(z):
    """Mean excitation energy of an element in eV: 19.2 for hydrogen, 12 Z + 7 below Z = 13, 9.76 Z + 58.8 Z^-0.19 from there."""
    if z == 1:
        return 19.2
    if z < 13:
        return 12.0 * z + 7.0
    return 9.76 * z + 58.8 * z ** -0.19


def element_radiation_length(z, a):
    """X0 of an element in g/cm^2: 716.4 A / (Z (Z + 1) ln(287 / sqrt(Z)))."""
    return 716.4 * a / (z * (z + 1.0) * np.log(287.0 / np.sqrt(z)))


def bethe(ke, mass, z, z_over_a, density, excitation_mev):
    """Mean stopping power of a heavy particle, MeV/mm (float64): K z^2 <Z/A> rho / beta^2 [1/2 ln(2 me beta^2 gamma^2 Tmax /
    I^2) - beta^2], without density-effect or shell correction.  Negative where the bracket is."""
    gamma = 1.0 + ke / mass
    beta2 = 1.0 - 1.0 / (gamma * gamma)
    bg2 = beta2 * gamma * gamma
    me = ELECTRON_MASS
    tmax = 2.0 * me * bg2 / (1.0 + 2.0 * gamma * me / mass + (me / mass) ** 2)
    bracket = 0.5 * np.log(2.0 * me * bg2 * tmax / excitation_mev ** 2) - beta2
    return 0.1 * K_BETHE * z * z * z_over_a * density / beta2 * bracket


def electron_collision(ke, z_over_a, density, excitation_mev):
    """Mean collision loss of an electron (Moller; Rohrlich and Carlson), MeV/mm (float64)."""
    me = ELECTRON_MASS
    tau = ke / me
    gamma = 1.0 + tau
    beta2 = 1.0 - 1.0 / (gamma * gamma)
    bracket = (np.log(tau * tau * (tau + 2.0) / (2.0 * (excitation_mev / me) ** 2)) + 1.0 - beta2 +
               (tau * tau / 8.0 - (2.0 * tau + 1.0) * np.log(2.0)) / (tau + 1.0) ** 2)
    return 0.1 * 0.5 * K_BETHE * z_over_a * density / beta2 * bracket


def below_peak(ke, s):
    """``s`` (a formula's values at the rising nodes ``ke``) with the nodes below the node the formula is largest at replaced
    by S_peak sqrt(ke / ke_peak): the formulas go negative down there."""
    peak = int(np.argmax(s))
    out = np.array(s, dtype=np.float64)
    out[:peak] = s[peak] * np.sqrt(ke[:peak] / ke[peak])
    return out


class StoppingMedia(object):
    """The stopping-power tables of several materials, a row per material: ``stopping_power[m][species][j]`` (MeV/mm,
    float32) at ``ke[j] = ke_min exp(j h)``, ``radiation_length[m]`` (mm; inf for vacuum) and ``birks[m]`` (mm/MeV).

    Built in float64 from ``Material.density`` (g/cm^3) and ``Material.composition`` (mass fractions by element symbol):
    Bethe's formula for mu, pi, K, p and alpha; Moller collision loss plus the mean radiative loss ``(ke + me) / X0`` for
    electrons and positrons; below the node at which a row's (collision) formula is largest, ``S_peak sqrt(ke / ke_peak)``.
    The mean excitation energy of a compound is Bragg's sum, ``excitation_energy={material name: eV}`` overrides it.
    A material of density 0 or without composition is vacuum: an all-zero row and an infinite radiation length.

    Defaults: 513 nodes from 1 keV to 100 GeV (h = ln(1e8) / 512, about 3.6 % per node): linear interpolation in log ke
    between them is off by less than 1e-3 of S anywhere on these rows.  ``desc`` is the chroma_stopping_media_desc over the
    arrays."""

    def __init__(self, materials, ke_min=1e-3, ke_max=1e5, nodes=513, excitation_energy=None, birks=None):
        self.materials = list(materials)
        if not self.materials:
            raise ValueError('stopping media: no material')
        if not (0 < ke_min < ke_max) or nodes < 2:
            raise ValueError('stopping media: need 0 < ke_min < ke_max and at least 2 nodes')
        excitation_energy, birks = dict(excitation_energy or {}), dict(birks or {})
        self.ke_min, self.nodes = float(ke_min), int(nodes)
        self.log_step = float(np.log(ke_max / ke_min) / (nodes - 1))
        self.ke = self.ke_min * np.exp(np.arange(self.nodes) * self.log_step)
        nm = len(self.materials)
        table = np.zeros((nm, len(SPECIES), self.nodes), dtype=np.float64)
        x0 = np.full(nm, np.inf, dtype=np.float64)
        self.excitation_energy = np.zeros(nm)          # eV
        for m, material in enumerate(self.materials):
            density, composition = float(getattr(material, 'density', 0.0) or 0.0), getattr(material, 'composition', None) or {}
            if density < 0:
                raise ValueError('material %s: negative density' % material.name)
            if density == 0 or not composition:
                continue
            z_over_a, log_i, inv_x0 = 0.0, 0.0, 0.0
            for symbol, w in composition.items():
                if symbol not in ELEMENTS:
                    raise ValueError('material %s: unknown element %r' % (material.name, symbol))
                z, a = ELEMENTS[symbol]
                z_over_a += w * z / a
                log_i += w * z / a * np.log(element_excitation_energy(z))
                inv_x0 += w / element_radiation_length(z, a)
            i_ev = float(excitation_energy.get(material.name, np.exp(log_i / z_over_a)))
            self.excitation_energy[m] = i_ev
            x0[m] = 10.0 / (density * inv_x0)
            for row, (mass, charge) in enumerate(zip(SPECIES_MASS, SPECIES_CHARGE)):
                if row == 0:
                    table[m, row] = below_peak(self.ke, electron_collision(self.ke, z_over_a, density, i_ev * 1e-6)) + (self.ke + ELECTRON_MASS) / x0[m]
                else:
                    table[m, row] = below_peak(self.ke, bethe(self.ke, mass, charge, z_over_a, density, i_ev * 1e-6))
        if not np.isfinite(table).all() or (table < 0).any():
            raise ValueError('stopping media: a table row is negative or not finite')
        self.stopping_power = np.ascontiguousarray(table, dtype=np.float32)
        self.radiation_length = x0.astype(np.float32)
        self.birks = np.array([float(birks.get(material.name, 0.0)) for material in self.materials], dtype=np.float32)
        if not np.isfinite(self.stopping_power).all() or (self.birks < 0).any() or not np.isfinite(self.birks).all() or not (self.radiation_length > 0).all():
            raise ValueError('stopping media: a row is negative or not finite')
        d = self.desc = _lib.StoppingMediaDesc()
        d.nmedia, d.nke, d.ke_min, d.log_step = nm, self.nodes, self.ke_min, self.log_step
        d.stopping_power, d.radiation_length, d.birks = _lib.ptr(self.stopping_power), _lib.ptr(self.radiation_length), _lib.ptr(self.birks)

    @classmethod
    def from_geometry(cls, geometry, **kwargs):
        """A row per material of ``geometry.unique_materials``, in that order: the rows of ``LightMedia.from_geometry`` and
        the material indices the geometry's triangles carry."""
        return cls(geometry.unique_materials, **kwargs)

    def __len__(self):
        return len(self.materials)

    def index(self, material):
        """The row of ``material`` (by identity), or -1."""
        for m, have in enumerate(self.materials):
            if have is material:
                return m
        return -1

    def interpolate(self, medium, species, ke):
        """S (MeV/mm, float64) of row (medium, species) at ``ke``: the table read as the device reads it, in double precision."""
        x = np.clip(np.log(np.asarray(ke, dtype=np.float64) / self.ke_min) / self.log_step, 0.0, self.nodes - 1.0)
        return np.interp(x, np.arange(self.nodes), self.stopping_power[medium, species].astype(np.float64))


class Stepper(object):
    """A StoppingMedia and the step control: at most ``max_steps`` steps per particle, each at most ``max_step`` mm long and
    losing at most the fraction ``max_loss`` of the kinetic energy; a particle that would fall below ``ke_cut`` MeV deposits
    the rest and stops.  ``scatter``: Highland multiple scattering.  ``outside``: the medium row of a particle with no
    triangle ahead of it (-1: none, such a particle has LEFT); without a geometry, the row of every particle."""

    def __init__(self, media, max_steps=1000, max_step=10.0, max_loss=0.05, ke_cut=0.05, scatter=True, outside=-1):
        self.media = media
        self.max_steps, self.max_step, self.max_loss, self.ke_cut = int(max_steps), float(max_step), float(max_loss), float(ke_cut)
        self.scatter, self.outside = bool(scatter), int(outside)
        if self.max_steps < 1 or not self.max_step > 0 or not 0 < self.max_loss <= 1 or self.ke_cut < 0 or self.outside < -1:
            raise ValueError('stepper: need max_steps >= 1, max_step > 0, 0 < max_loss <= 1, ke_cut >= 0, outside >= -1')

    def options(self, outside=None):
        o = _lib.ParticleOptions()
        o.max_steps, o.max_step, o.max_loss, o.ke_cut = self.max_steps, self.max_step, self.max_loss, self.ke_cut
        o.scatter, o.outside = int(self.scatter), self.outside if outside is None else int(outside)
        return o

    def expected_photons_at_most(self, vertices, light_media):
        """A cheap upper bound of the photons the tracks of ``vertices`` emit, for cutting batches: every particle loses all
        its kinetic energy, Cherenkov light at beta = 1 in the medium of the largest yield per mm over a path of ke / S_min
        (S_min: the smallest non-zero stopping power of its species over all media and energies up to ke), plus scintillation
        of the largest light yield on the whole of ke (unquenched)."""
        total = 0.0
        probe = Segments([[0, 0, 0]], [[0, 0, 1]], 0, 0, 1.0, 1.0, 1.0, 0)          # 1 mm at beta = 1, z = 1, 1 MeV
        per = light_media.expected_per_segment(probe)[:, 0]                           # Cherenkov per mm + yield per MeV
        yields = np.array([s.light_yield for s in light_media.sources], dtype=np.float64)
        cherenkov_per_mm, yield_max = float((per - yields).max()), float(yields.max())
        for v in _as_list(vertices):
            code = _pdg_code(v)
            row = SPECIES.get(abs(code)) if code is not None else None
            ke = float(v.ke)
            if row is None or not ke > 0:
                continue
            s = self.media.stopping_power[:, row, :][:, self.media.ke <= max(ke, self.media.ke[0])].astype(np.float64)
            s = s[s > 0]
            path = ke / s.min() if len(s) else 0.0
            path = min(path, self.max_steps * self.max_step)
            total += SPECIES_CHARGE[row] ** 2 * cherenkov_per_mm * path + yield_max * ke
        return total


def _as_list(vertices):
    return [vertices] if isinstance(vertices, event.Vertex) else list(vertices)


def _pdg_code(vertex):
    return vertex.pdgcode if vertex.pdgcode is not None else PDG_CODES.get(vertex.particle_name)


class ParticleState(object):
    """The particles of one call as NumPy arrays (the fields of chroma_particle_arrays), from vertices."""
    FIELDS = (('pos', np.float32), ('dir', np.float32), ('ke', np.float32), ('t', np.float32), ('last_hit', np.int32), ('species', np.int32),
              ('z', np.float32), ('mass', np.float32), ('evidx', np.uint32), ('nsteps', np.uint32), ('rng_counter', np.uint32),
              ('status', np.uint32))

    def __init__(self, vertices, evidx=0, particle_base=0):
        vertices = _as_list(vertices)
        n = len(vertices)
        self.n, self.particle_base = n, int(particle_base)
        self.pos = np.ascontiguousarray([np.asarray(v.pos, dtype=np.float64) for v in vertices], dtype=np.float32).reshape(n, 3)
        d = np.array([np.asarray(v.dir, dtype=np.float64) for v in vertices], dtype=np.float64).reshape(n, 3)
        with np.errstate(invalid='ignore', divide='ignore'):
            d = d / np.linalg.norm(d, axis=1)[:, None]
        self.dir = np.ascontiguousarray(d, dtype=np.float32)
        self.ke = np.array([v.ke for v in vertices], dtype=np.float32)
        self.t = np.array([v.t0 for v in vertices], dtype=np.float32)
        self.last_hit = np.full(n, -1, dtype=np.int32)
        self.species = np.full(n, -1, dtype=np.int32)
        self.z, self.mass = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
        for i, v in enumerate(vertices):
            code = _pdg_code(v)
            if code in PARTICLES and abs(code) in SPECIES:
                self.species[i] = SPECIES[abs(code)]
                self.mass[i], self.z[i] = PARTICLES[code]
        self.evidx = np.ascontiguousarray(np.broadcast_to(np.asarray(evidx, dtype=np.uint32), (n,)))
        self.nsteps, self.rng_counter = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
        self.status = np.zeros(n, dtype=np.uint32)

    def struct(self, pointers=None):
        """chroma_particle_arrays over these host arrays, or over ``pointers`` (name -> device pointer)."""
        s = _lib.ParticleArrays()
        for name, _ in self.FIELDS:
            setattr(s, name, pointers[name] if pointers is not None else _lib.ptr(getattr(self, name)))
        s.n, s.particle_base = self.n, self.particle_base
        return s


POINT_FIELDS = (('pos', np.float32, 3), ('t', np.float32, 1), ('dir', np.float32, 3), ('ke', np.float32, 1), ('edep', np.float32, 1),
                ('qedep', np.float32, 1), ('medium', np.int32, 1))


def point_arrays(rows, fill=0):
    """name -> a host array of ``rows`` step points, and the chroma_particle_points over them"""
    arrays = {name: np.full((rows, width) if width > 1 else (rows,), fill, dtype=dtype) for name, dtype, width in POINT_FIELDS}
    return arrays, point_struct({name: _lib.ptr(a) for name, a in arrays.items()})


def point_struct(pointers):
    s = _lib.ParticlePoints()
    for name, _, _ in POINT_FIELDS:
        setattr(s, name, pointers[name])
    return s


class Tracks(object):
    """The step points of n particles as flat arrays in particle order: ``pos``, ``dir`` float32 (N, 3); ``t``, ``ke`` (left
    after the step), ``edep``, ``qedep`` float32 (N,); ``medium`` int32 (N,) (-1 for a vertex point); the points of particle i
    are ``offsets[i] .. offsets[i + 1]``.  Per particle: ``status`` (``STATUS``), ``z``, ``mass``, ``evidx``."""

    def __init__(self, points, offsets, state):
        for name, _, _ in POINT_FIELDS:
            setattr(self, name, points[name])
        self.offsets = np.asarray(offsets, dtype=np.uint32)
        self.status, self.z, self.mass, self.evidx = state.status, state.z, state.mass, state.evidx

    def __len__(self):
        return len(self.offsets) - 1

    def steps(self, i):
        """The ``event.Steps`` of particle i."""
        s = slice(int(self.offsets[i]), int(self.offsets[i + 1]))
        return event.Steps(self.pos[s, 0].copy(), self.pos[s, 1].copy(), self.pos[s, 2].copy(), self.t[s].copy(), self.dir[s, 0].copy(),
                           self.dir[s, 1].copy(), self.dir[s, 2].copy(), self.ke[s].copy(), self.edep[s].copy(), self.qedep[s].copy())

    def beta(self):
        """beta of every point in single precision, as the library forms it: sqrt(1 - 1/gamma^2), gamma = 1 + ke/mass."""
        f32 = np.float32
        mass = np.repeat(self.mass, np.diff(self.offsets.astype(np.int64)))
        with np.errstate(invalid='ignore', divide='ignore'):
            gamma = f32(1) + self.ke / mass
            return np.sqrt(f32(1) - f32(1) / (gamma * gamma), dtype=f32)

    def segments(self, segment_base=0):
        """(Segments, medium): the segments of the tracks in particle order, points k -> k + 1 of one particle, and the
        medium row of each (its end point's): what ``generator.steps.generate_photons`` takes with a LightMedia.  The same
        bits as chroma_particles_segments."""
        counts = np.diff(self.offsets.astype(np.int64))
        first, last = np.zeros(len(self.t), dtype=bool), np.zeros(len(self.t), dtype=bool)
        first[self.offsets[:-1][counts > 0]] = True
        last[(self.offsets[1:] - 1)[counts > 0]] = True
        b, a = ~first, ~last          # b: every point but a particle's first; a: every point but its last
        beta = self.beta()
        particle = np.repeat(np.arange(len(counts)), counts)
        segs = Segments(self.pos[a], self.pos[b], self.t[a], self.t[b], np.float32(0.5) * (beta[a] + beta[b]), self.z[particle[b]],
                        self.qedep[b], self.evidx[particle[b]], segment_base=segment_base)
        return segs, np.ascontiguousarray(self.medium[b])


def fill_steps(vertices, tracks):
    """Copies of ``vertices`` with ``steps`` those of ``tracks``."""
    out = []
    for i, v in enumerate(_as_list(vertices)):
        v = copy.copy(v)
        v.steps = tracks.steps(i)
        out.append(v)
    return out


def advance(state, stepper, seed, matrix_struct, distance=None, triangle=None, medium=None):
    """ONE iteration of the particles of ``state`` (a ParticleState, advanced in place) on the HOST
    (chroma_particles_advance_host), given per particle the nearest triangle along its direction (``distance`` float32,
    ``triangle`` int32; None: none ahead) and the medium row on its side of it (int32; None: ``stepper.outside``).  Points go
    to the step-major matrix ``matrix_struct`` (``point_arrays(n * (max_steps + 1))``)."""
    distance = None if distance is None else np.ascontiguousarray(distance, dtype=np.float32)
    triangle = None if triangle is None else np.ascontiguousarray(triangle, dtype=np.int32)
    medium = None if medium is None else np.ascontiguousarray(medium, dtype=np.int32)
    particles, options = state.struct(), stepper.options()
    _lib.check(_lib.load().chroma_particles_advance_host(ctypes.byref(stepper.media.desc), ctypes.byref(particles), ctypes.byref(options),
                                                         int(seed) & (2 ** 64 - 1), _lib.ptr(distance), _lib.ptr(triangle), _lib.ptr(medium),
                                                         ctypes.byref(matrix_struct)))


def track(vertices, stepper, seed, particle_base=0, medium=0, evidx=0):
    """The tracks of ``vertices`` in ONE medium, row ``medium`` of the stepper's table, made on the HOST: (the vertices with
    ``steps`` filled, copies; a :class:`Tracks`).  Particle i draws from the stream of ``particle_base + i``."""
    vertices = _as_list(vertices)
    state = ParticleState(vertices, evidx=evidx, particle_base=particle_base)
    lib = _lib.load()
    options = stepper.options(outside=medium)
    matrix, matrix_struct = point_arrays(state.n * (stepper.max_steps + 1))
    particles = state.struct()
    total = ctypes.c_uint64()
    seed = int(seed) & (2 ** 64 - 1)
    _lib.check(lib.chroma_particles_track_host(ctypes.byref(stepper.media.desc), ctypes.byref(particles), ctypes.byref(options), seed,
                                               ctypes.byref(matrix_struct), ctypes.byref(total)))
    flat, flat_struct = point_arrays(total.value)
    offsets = np.zeros(state.n + 1, dtype=np.uint32)
    _lib.check(lib.chroma_particles_points_host(ctypes.byref(particles), stepper.max_steps, ctypes.byref(matrix_struct), ctypes.byref(flat_struct),
                                                _lib.ptr(offsets), total.value))
    tracks = Tracks(flat, offsets, state)
    return fill_steps(vertices, tracks), tracks
