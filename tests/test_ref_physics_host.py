"""The CPU oracle against the reference's OWN physics and DAQ sources, bit for bit, without a GPU.

oracle/_ref/libchroma_ref_physics_{libm,contract}.so are chroma/cuda/propagate.cu (+ photon.h, random.h, cx.h, mesh.h ...)
and chroma/cuda/daq.cu compiled for the host by oracle/ref_physics_driver.cc over the stand-in headers of oracle/ref_shim.
Every other parity test of the HIP engine has oracle/chroma_oracle.c as its comparand; here that comparand is held to the
statements it restates: which branch, which rescaling, which clamp, which statement draws and in what order.

Every comparison is made twice -- reference(libm) against oracle(libm), reference(contract) against oracle(contract) -- and is
bit for bit on pos, dir, pol, wavelengths, t, flags, last_hit_triangles, weights, evidx and the draw counters.  Two NaNs count
as equal; there is no other tolerance.  The generator, the mapping of a word to (0, 1] and the Box-Muller deviate are the
project's own contract on both sides (oracle/ref_shim/curand_kernel.h) and are not what these tests pin.

The numeric floors (flag unions, at least 100 photons per surface model, more than one launch, outcomes that must occur) are
properties of the INPUTS, evaluated on the oracle's result alone: they keep a case from passing empty.

The tests skip only where oracle/_ref holds no physics libraries (no reference tree at build time).
"""
import functools

import numpy as np
import pytest

from chroma_amd import event
from chroma_amd.event import Photons
from conftest import bomb, make_stress_geometry
from test_gpu_fuzz import _random_optics

VARIANTS = ('libm', 'contract')
FIELDS = ('pos', 'dir', 'pol', 'wavelengths', 't', 'flags', 'last_hit_triangles', 'weights', 'evidx')
RANDOM_OPTICS_SEEDS = (101, 102, 103, 104)               # the seeds of test_gpu_fuzz.test_random_optics
SETTINGS = {'plain': {}, 'weights': dict(use_weights=True), 'scatter_first+1': dict(scatter_first=1),
            'scatter_first-1': dict(scatter_first=-1)}
WAVELENGTHS = {'400nm': (400.0, None), '300-700nm': (300.0, 700.0)}
TERMINAL = (event.NO_HIT, event.BULK_ABSORB, event.SURFACE_DETECT, event.SURFACE_ABSORB, event.NAN_ABORT)
BREAK, CONTINUE, PASS = 0, 1, 2
Z = (0.0, 0.0, 1.0)


@pytest.fixture(scope='module')
def ref(oracle_mod):
    """The oracle module, once both builds of the reference's physics are there."""
    if not oracle_mod.have_ref_physics():
        pytest.skip('oracle/_ref holds no physics libraries (they need the reference tree at build time)')
    for v in VARIANTS:
        assert oracle_mod.load_ref_physics(v) is not None
    return oracle_mod


# ---- comparing ------------------------------------------------------------------------------------------------------------------
def differing(got, want, got_counters=None, want_counters=None):
    """Per photon: does any field differ?  Floats by their bits, except that a NaN equals a NaN."""
    n = len(want.pos)
    bad = np.zeros(n, dtype=bool)
    per_field = {}
    for name in FIELDS:
        a, b = np.ascontiguousarray(getattr(got, name)), np.ascontiguousarray(getattr(want, name))
        assert a.dtype == b.dtype and a.shape == b.shape, name
        if a.dtype == np.float32:
            same = (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
        else:
            same = a == b
        d = ~same.reshape(n, -1).all(axis=1)
        per_field[name] = int(d.sum())
        bad |= d
    if want_counters is not None:
        d = np.asarray(got_counters) != np.asarray(want_counters)
        per_field['counters'] = int(d.sum())
        bad |= d
    return bad, per_field


def assert_same(got, want, got_counters, want_counters, what):
    bad, per_field = differing(got, want, got_counters, want_counters)
    assert not bad.any(), '%s: %d of %d photons differ (first: %d); per field %s' % (
        what, bad.sum(), len(bad), np.flatnonzero(bad)[0], {k: v for k, v in per_field.items() if v})


# ---- geometries -----------------------------------------------------------------------------------------------------------------
GEOMETRIES = ('tiny', 'stress') + tuple('optics%d' % s for s in RANDOM_OPTICS_SEEDS)


@functools.lru_cache(maxsize=None)
def world(name):
    from chroma_amd import demo
    from chroma_amd.loader import create_geometry_from_obj
    from chroma_amd.gpu.geometry import pack_geometry
    if name == 'tiny':
        geometry = create_geometry_from_obj(demo.tiny())
    elif name == 'stress':
        geometry = make_stress_geometry()
    elif name == 'single':
        geometry = create_geometry_from_obj(_single_routines_detector())
    else:
        geometry = create_geometry_from_obj(_random_optics(int(name[len('optics'):])))
    return geometry, pack_geometry(geometry)


@functools.lru_cache(maxsize=None)
def oracle_history(geometry_name, setting, wavelength, max_steps=100, variant='contract'):
    """The oracle's end state of the 8000-photon case: computed once, shared by the comparison and the preconditions."""
    import oracle
    lo, hi = WAVELENGTHS[wavelength]
    ph = bomb(8000, 3, wavelength=lo, wavelength_hi=hi)
    end, counters, stats = oracle.propagate(world(geometry_name)[1], ph, seed=7, max_steps=max_steps, variant=variant, **SETTINGS[setting])
    return ph, end, counters, stats


# ---- full histories ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('wavelength', sorted(WAVELENGTHS))
@pytest.mark.parametrize('setting', sorted(SETTINGS))
@pytest.mark.parametrize('geometry_name', GEOMETRIES)
def test_full_histories(ref, geometry_name, setting, wavelength):
    """8000 photons to the end (100 steps): the oracle's end state is the reference kernel's, in both builds."""
    packed = world(geometry_name)[1]
    for variant in VARIANTS:
        ph, want, want_counters, _ = oracle_history(geometry_name, setting, wavelength, variant=variant)
        got, got_counters, _ = ref.ref_propagate(packed, ph, seed=7, max_steps=100, variant=variant, **SETTINGS[setting])
        assert_same(got, want, got_counters, want_counters, '%s, %s, %s, %s' % (geometry_name, setting, wavelength, variant))
        assert want_counters.max() > 0


@pytest.mark.parametrize('max_steps', [1, 10])
@pytest.mark.parametrize('setting', sorted(SETTINGS))
def test_histories_cut_short(ref, setting, max_steps):
    """The stress geometry again, stopped after 1 and after 10 steps: photons are left alive, mid-history."""
    packed = world('stress')[1]
    for variant in VARIANTS:
        ph, want, want_counters, _ = oracle_history('stress', setting, '300-700nm', max_steps=max_steps, variant=variant)
        got, got_counters, _ = ref.ref_propagate(packed, ph, seed=7, max_steps=max_steps, variant=variant, **SETTINGS[setting])
        assert_same(got, want, got_counters, want_counters, 'stress, %s, %d steps, %s' % (setting, max_steps, variant))
    if max_steps == 1:
        assert np.count_nonzero((want.flags & event.TERMINAL_MASK) == 0) > 1000


def _surface_model_of_triangle(packed):
    codes = packed.arrays['material_codes']
    surface = ((codes >> 8) & 0xFF).astype(np.int64)
    model = np.full(len(codes), -1, dtype=np.int64)
    has = surface < len(packed.arrays['surf_model'])            # (0xFF: no surface)
    model[has] = packed.arrays['surf_model'][surface[has]]
    return model


@pytest.mark.parametrize('geometry_name', [g for g in GEOMETRIES if g != 'tiny'])
def test_the_histories_reach_every_branch(ref, geometry_name):
    """Preconditions of test_full_histories on the stress cube and on the random optics, from the oracle's results over the
    eight cases of a geometry: every history bit of 0x3fe occurs, and each of the four surface models (default, thin film,
    WLS, dichroic) ends at least 100 photons ON a triangle that carries it (a surface absorption or detection there)."""
    packed = world(geometry_name)[1]
    model_of = _surface_model_of_triangle(packed)
    union = 0
    ended = np.zeros(4, dtype=np.int64)
    for setting in SETTINGS:
        for wavelength in WAVELENGTHS:
            _, end, _, _ = oracle_history(geometry_name, setting, wavelength)
            union |= int(np.bitwise_or.reduce(end.flags))
            at_surface = ((end.flags & (event.SURFACE_ABSORB | event.SURFACE_DETECT)) != 0) & (end.last_hit_triangles >= 0)
            models = model_of[end.last_hit_triangles[at_surface]]
            ended += np.bincount(models[models >= 0], minlength=4)[:4]
    assert union & 0x3FE == 0x3FE, hex(union)
    assert (ended >= 100).all(), ended


# ---- the launch policy ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('use_weights', [False, True])
@pytest.mark.parametrize('geometry_name', ['tiny', 'stress'])
def test_launch_policy(ref, geometry_name, use_weights):
    """20000 photons: one step per launch while 8192 are alive and weights are off (every launch normalises direction and
    polarisation again on load, propagate.cu:248,250), all steps in one launch with weights."""
    packed = world(geometry_name)[1]
    ph = bomb(20000, 11, wavelength=300.0, wavelength_hi=700.0)
    for variant in VARIANTS:
        want, want_counters, stats = ref.propagate(packed, ph, seed=21, max_steps=100, use_weights=use_weights, nthreads=4, variant=variant)
        got, got_counters, rstats = ref.ref_propagate(packed, ph, seed=21, max_steps=100, use_weights=use_weights, variant=variant)
        assert_same(got, want, got_counters, want_counters, '%s, 20000 photons, weights %s, %s' % (geometry_name, use_weights, variant))
        assert rstats['launches'] == stats['launches']
        assert stats['launches'] == 1 if use_weights else stats['launches'] > 1, stats['launches']


# ---- entry edges --------------------------------------------------------------------------------------------------------------------
def _edge_batch(packed):
    """Plain photons as controls, and one block of rows per edge of the issue's table; the blocks overlap where noted."""
    d = packed.desc
    ph = bomb(6000, 29, wavelength=300.0, wavelength_hi=700.0)
    n = len(ph)
    counters = np.zeros(n, dtype=np.uint32)
    rows = {}

    def block(name, start, count):
        rows[name] = slice(start, start + count)
        return rows[name]
    s = block('nan position', 100, 30)
    ph.pos[s][np.arange(30), np.arange(30) % 3] = np.nan
    s = block('zero direction', 200, 30)
    ph.dir[s] = 0.0
    s = block('unnormalised', 300, 200)
    ph.dir[s] *= np.repeat([2.5, 0.3, 1e-3, 1e4], 50)[:, None].astype(np.float32)
    ph.pol[s] *= np.tile([0.1, 7.0], 100)[:, None].astype(np.float32)
    s = block('terminal flags', 450, 100)                   # (its first half is unnormalised too: rows 3 and 4 combined)
    ph.flags[s] = np.tile(np.array(TERMINAL, dtype=np.uint32), 20)
    ph.flags[540:550] |= event.RAYLEIGH_SCATTER | event.BULK_REEMIT
    s = block('last hit set', 600, 400)
    ph.last_hit_triangles[s] = np.arange(400) % d.ntriangles
    s = block('counters', 900, 300)                          # (its first third has a last hit too: rows 5 and 6 combined)
    counters[s] = np.tile(np.array([3, 4, 2 ** 20 + 1], dtype=np.uint32), 100)
    s = block('weights', 1300, 300)
    ph.weights[s] = np.tile(np.array([0.0, 1e-9, 1.0], dtype=np.float32), 100)
    s = block('outside the world', 1700, 100)
    ph.pos[s] = 1e6
    ph.dir[1700:1750] = [1.0, 0.0, 0.0]
    ph.dir[1750:1800] = [-1.0, -1.0, -1.0]
    lo = np.float32(d.wavelength_start)
    hi = np.float32(d.wavelength_start + (d.wavelength_n - 1) * d.wavelength_step)
    ends = [np.nextafter(lo, np.float32(0)), lo - np.float32(7.5), lo, np.nextafter(lo, np.float32(1e9)), lo + np.float32(0.5),
            np.nextafter(hi, np.float32(0)), hi - np.float32(0.5), hi, np.nextafter(hi, np.float32(1e9)), hi + np.float32(300.0)]
    s = block('table ends', 2000, 400)
    ph.wavelengths[s] = np.tile(np.array(ends, dtype=np.float32), 40)
    ph.weights[2200:2400] = np.float32(1e-9)                 # (rows 7 and 9 combined)
    return ph, counters, rows


@pytest.mark.parametrize('setting', sorted(SETTINGS))
@pytest.mark.parametrize('geometry_name', ['tiny', 'stress'])
def test_entry_edges(ref, geometry_name, setting):
    packed = world(geometry_name)[1]
    ph, counters, rows = _edge_batch(packed)
    for variant in VARIANTS:
        want, want_counters, _ = ref.propagate(packed, ph, seed=5, max_steps=100, rng_counters=counters, variant=variant, **SETTINGS[setting])
        got, got_counters, _ = ref.ref_propagate(packed, ph, seed=5, max_steps=100, rng_counters=counters, variant=variant, **SETTINGS[setting])
        assert_same(got, want, got_counters, want_counters, '%s, %s, edge batch, %s' % (geometry_name, setting, variant))
    # what the rows must have been, on the oracle's result
    nan_abort = np.uint32(event.NO_HIT | event.NAN_ABORT)
    assert (want.flags[rows['nan position']] == nan_abort).all() and (want.flags[rows['zero direction']] == nan_abort).all()
    s = rows['terminal flags']
    assert np.array_equal(want.flags[s], ph.flags[s]) and np.array_equal(want.dir[s], ph.dir[s])       # untouched, not even normalised
    assert np.array_equal(want_counters[s], counters[s])
    assert (want.flags[1700:1750] == event.NO_HIT).all()
    assert (want_counters[rows['counters']] > counters[rows['counters']]).all()
    ended = (want.flags[rows['table ends']] & event.TERMINAL_MASK) != 0
    assert ended.sum() > 300 and (want_counters[rows['table ends']] > 0).all()


# ---- single routines ----------------------------------------------------------------------------------------------------------------
def _single_routines_detector():
    """One cube for the single-routine tests: materials with 0 (vacuum), 1 and 3 re-emission components and, on its
    triangles, films of thickness 0 and 1 mm (exp overflows), a film that does not transmit, a film and a default surface that detect nothing, WLS surfaces that never and
    always re-emit, dichroic tables of five angles and of ONE, and a default surface."""
    from chroma_amd.geometry import Solid, Material, Surface, DichroicProps, vacuum, standard_wavelengths
    from chroma_amd.detector import Detector
    from chroma_amd.make import box
    wl = standard_wavelengths.astype(float)
    cdf = np.clip((wl - 400.0) / 100.0, 0.0, 1.0)
    tgrid = np.arange(0, 1000, 0.05)

    def scintillator(name, ncomp):
        m = Material(name)
        m.set('refractive_index', 1.5); m.set('absorption_length', 50.0); m.set('scattering_length', 200.0)
        for k in range(ncomp):
            tc = 1.0 - np.exp(-tgrid / (3.0 + 4.0 * k)); tc /= tc[-1]
            p = Material('tmp'); p.set('x', (0.8, 0.3, 0.6)[k]); m.comp_reemission_prob.append(p.x)
            c = Material('tmp'); c.set('x', cdf); m.comp_reemission_wvl_cdf.append(c.x)
            m.comp_reemission_time_cdf.append(np.column_stack([tgrid, tc]).astype(np.float32))
            a = Material('tmp'); a.set('x', (100.0, 150.0, 300.0)[k] * ncomp / 1.5); m.comp_absorption_length.append(a.x)
        return m

    def film(name, thickness, transmissive, detect=0.3):
        s = Surface(name, model=1)
        s.set('detect', detect); s.set('eta', 2.0); s.set('k', 1.5); s.set('reflect_diffuse', 0.2)
        s.thickness = thickness; s.transmissive = transmissive
        return s

    def wls(name, reemit):
        s = Surface(name, model=2)
        s.set('absorb', 0.5); s.set('reemit', reemit); s.set('reflect_specular', 0.1); s.set('reflect_diffuse', 0.1)
        s.set('reemission_cdf', cdf)
        return s

    def dichroic(name, angles):
        s = Surface(name, model=3)
        refl = [np.column_stack([wl, np.clip(0.2 + 0.1 * k + (wl - 300) / 2000.0, 0, 0.9)]) for k in range(len(angles))]
        tran = [np.column_stack([wl, np.clip(0.6 - 0.1 * k - (wl - 300) / 4000.0, 0, 0.9) * 0.9]) for k in range(len(angles))]
        s.dichroic_props = DichroicProps(np.asarray(angles, dtype=float), refl, tran)
        return s
    pmt = Surface('default')
    pmt.set('detect', 0.4); pmt.set('absorb', 0.2); pmt.set('reflect_diffuse', 0.2); pmt.set('reflect_specular', 0.1)
    # (with weights a surface that detects ends the photon before its draw, photon.h:556,711: the rescaled reflection and
    #  transmission probabilities decide only on surfaces that detect nothing)
    blind = Surface('default_blind')
    blind.set('absorb', 0.3); blind.set('reflect_diffuse', 0.3); blind.set('reflect_specular', 0.2)
    faces = [film('film_blind', 20e-6, 1, detect=0.0), blind, film('film0', 0.0, 1), film('film_thick', 1.0, 1), film('film_opaque', 20e-6, 0), film('film', 20e-6, 1),
             wls('wls_never', 0.0), wls('wls_always', 1.0),
             dichroic('dichroic1', [0.5]), dichroic('dichroic5', [0.2, 0.4, float(np.float32(np.arccos(0.5))), 1.2, 1.3]),
             dichroic('dichroic0', [0.0, 0.4, 0.8, 1.2, np.pi / 2]), pmt]
    mesh = box(200.0, 200.0, 200.0)
    surfaces = np.empty(len(mesh.triangles), dtype=object)
    for i in range(len(surfaces)):
        surfaces[i] = faces[i % len(faces)]
    black = Surface('black'); black.set('absorb', 1.0)
    scint3 = scintillator('scint3', 3)
    det = Detector(vacuum)
    det.add_pmt(Solid(mesh, scint3, vacuum, surface=surfaces))
    det.add_solid(Solid(box(50.0, 50.0, 50.0), scintillator('scint1', 1), scint3, surface=pmt))
    det.add_solid(Solid(box(2000.0, 2000.0, 2000.0), vacuum, vacuum, surface=black))
    return det


def _index(items, name):
    return [getattr(x, 'name', None) for x in items].index(name)


def one_photon(direction, polarization, wavelength=400.0, weight=1.0, position=(1.0, 2.0, 3.0), time=10.0):
    ph = Photons(np.array([position]), np.array([direction]), np.array([polarization]), np.array([wavelength]),
                 t=np.array([time]), weights=np.array([weight]))
    ph.last_hit_triangles[:] = 5
    return ph


def incoming(theta, azimuth=0.0):
    """Direction of a photon that meets the surface with normal +z under the angle theta (double, then rounded once)."""
    return np.array([np.sin(theta) * np.cos(azimuth), np.sin(theta) * np.sin(azimuth), -np.cos(theta)], dtype=np.float64).astype(np.float32)


def s_and_p(direction):
    """Unit polarisations across the plane of incidence (s) and in it (p), for a direction in the xz plane."""
    d = direction.astype(np.float64)
    return np.array([0.0, 1.0, 0.0]), np.array([-d[2], 0.0, d[0]]) / np.hypot(d[0], d[2])


def both_single(ref, packed, which, photon, what, **kw):
    """One call of a routine by the reference and by the oracle, in both builds: same photon, same counter, same command.
    Returns the contract oracle's (photon, counter, command)."""
    for variant in VARIANTS:
        want = ref.single(packed, which, photon, variant=variant, **kw)
        got = ref.ref_single(packed, which, photon, variant=variant, **kw)
        assert_same(got[0], want[0], [got[1]], [want[1]], '%s, %s, %s' % (which, what, variant))
        assert got[2] == want[2], '%s, %s, %s: command %d, the oracle %d' % (which, what, variant, got[2], want[2])
    return want


def test_propagate_at_boundary_edges(ref):
    """Fresnel at a bare boundary: normal incidence (the plane normal is then the polarisation, photon.h:322-323), the critical
    angle of 1.5 -> 1.0 stepped through ulp by ulp and beyond (a NaN refracted angle forces the reflection, photon.h:335,350),
    equal indices, grazing incidence; polarisation across and in the plane of incidence, and between the two."""
    packed = world('single')[1]
    critical = np.float32(np.arcsin(1.0 / 1.5))
    near_critical = [critical]
    for _ in range(3):
        near_critical = [np.nextafter(near_critical[0], np.float32(0))] + near_critical + [np.nextafter(near_critical[-1], np.float32(9))]
    cases = [('normal incidence', incoming(0.0), 1.5, 1.0), ('normal incidence, into the denser', incoming(0.0), 1.0, 1.5),
             ('all but normal', incoming(3e-7), 1.5, 1.0), ('nearly normal', incoming(2e-6), 1.5, 1.0)]
    cases += [('critical angle %+d ulp' % (k - 3), incoming(np.float64(a)), 1.5, 1.0) for k, a in enumerate(near_critical)]
    cases += [('beyond the critical angle, %.2f' % a, incoming(a), 1.5, 1.0) for a in (0.75, 1.0, 1.3, 1.5)]
    cases += [('equal indices, %.2f' % a, incoming(a), 1.33, 1.33) for a in (0.0, 0.4, 1.2)]
    cases += [('grazing, pi/2 - %g' % e, incoming(np.pi / 2 - e), n1, n2) for e in (1e-3, 1e-5, 1e-7) for n1, n2 in ((1.0, 1.5), (1.5, 1.0))]
    cases += [('below the critical angle, %.2f' % a, incoming(a), 1.5, 1.0) for a in (0.3, 0.6, 0.72)]
    ncalls = 0
    outcome = {}
    for what, direction, n1, n2 in cases:
        s, p = s_and_p(direction)
        for pname, pol in (('s', s), ('p', p), ('mixed', (s + p) / np.sqrt(2.0))):
            for photon_id in range(4):
                end, counter, command = both_single(ref, packed, 'propagate_at_boundary', one_photon(direction, pol), '%s, %s' % (what, pname),
                                                    seed=3, photon_id=photon_id, normal=Z, n1=n1, n2=n2)
                assert counter == 2 and command == -1
                outcome.setdefault(what, []).append(bool(end.flags[0] & event.REFLECT_SPECULAR))
                ncalls += 1
    assert ncalls >= 300
    for what, reflected in outcome.items():
        if what.startswith('beyond') or what.endswith('+3 ulp'):
            assert all(reflected), what                       # total reflection
        if what.startswith('equal indices'):
            assert not any(reflected), what                   # nothing to reflect from
    below = sum((outcome[w] for w in outcome if w.startswith('below')), [])
    assert any(below) and not all(below)


@functools.lru_cache(maxsize=None)
def extreme_counters(seed=1, photon_id=0, want=4):
    """Counters of the stream (seed, photon_id) at which the NEXT uniform is below 2^-20, and above 1 - 2^-20."""
    import oracle
    low, high = [], []
    chunk = 1 << 22
    for start in range(0, 1 << 27, chunk):
        u = oracle.uniform_stream(seed, photon_id, chunk, start=start)
        low += (start + np.flatnonzero(u < 2.0 ** -20)).tolist()
        high += (start + np.flatnonzero(u > 1.0 - 2.0 ** -20)).tolist()
        if len(low) >= want and len(high) >= want:
            break
    assert len(low) >= want and len(high) >= want
    return tuple(low[:want]), tuple(high[:want])


def test_rayleigh_and_diffuse_at_extreme_draws(ref):
    """rayleigh_scatter and the diffuse reflector where a draw is all but 0 or all but 1: cos(theta) = -1 and +1 (the
    `1 - |cos| < 1e-6` branch, photon.h:181), a sphere point at a pole; and the ordinary draws around them."""
    packed = world('single')[1]
    low, high = extreme_counters()
    starts = sorted(set(c - back for c in low + high for back in (0, 1, 2, 3) if c - back >= 0)) + list(range(40))
    pols = [np.array([0.0, 0.0, 1.0]), np.array([0.0, 0.0, -1.0]), np.array([1.0, 0.0, 0.0]), np.array([0.6, 0.0, 0.8]),
            np.array([0.0, 0.0, 1.0000001]), np.array([3e-6, 0.0, 1.0]), np.array([0.36, 0.48, 0.8])]
    polar = 0
    for counter in starts:
        for pol in pols:
            end, after, command = both_single(ref, packed, 'rayleigh_scatter', one_photon(incoming(0.3), pol), 'counter %d' % counter,
                                              seed=1, photon_id=0, counter=counter)
            assert after == counter + 2
        if counter in low or counter in high:
            polar += 1
    assert polar == len(low) + len(high)
    normals = [Z, (0.0, 0.0, -1.0), (0.6, 0.0, 0.8), (1.0, 0.0, 0.0)]
    for counter in starts:
        for normal in normals:
            end, after, command = both_single(ref, packed, 'diffuse_reflector', one_photon(incoming(0.3), [0.0, 1.0, 0.0]),
                                              'counter %d' % counter, seed=1, photon_id=0, counter=counter, normal=normal)
            assert command == CONTINUE and after >= counter + 5 and (after - counter - 2) % 3 == 0
            assert end.flags[0] == event.REFLECT_DIFFUSE
    assert (len(pols) + len(normals)) * len(starts) >= 300


def test_specular_reflector(ref):
    packed = world('single')[1]
    for a in (0.0, 1e-7, 0.3, 1.0, 1.5, np.pi / 2 - 1e-6):
        for az in (0.0, 0.7, 2.0):
            end, after, command = both_single(ref, packed, 'specular_reflector', one_photon(incoming(a, az), [0.0, 1.0, 0.0]),
                                              'theta %g' % a, normal=Z, counter=9)
            assert command == CONTINUE and after == 9 and end.flags[0] == event.REFLECT_SPECULAR


def test_propagate_to_boundary_edges(ref):
    """Lengths of 1e-6 and 1e9, a boundary at distance 0, forced and forbidden first scatters, weights (alive and below
    the threshold), in materials with 0, 1 and 3 re-emission components."""
    geometry, packed = world('single')
    materials = {n: _index(geometry.unique_materials, name) for n, name in ((0, 'vacuum'), (1, 'scint1'), (3, 'scint3'))}
    assert [int(packed.arrays['mat_num_comp'][materials[n]]) for n in (0, 1, 3)] == [0, 1, 3]
    commands, flags = set(), 0
    ncalls = 0
    for ncomp, material in materials.items():
        for absorption in (1e-6, 50.0, 1e9):
            for scattering in (1e-6, 200.0, 1e9):
                for distance in (0.0, 100.0):
                    for scatter_first in (0, 1, -1):
                        for use_weights, weight in ((False, 1.0), (True, 1.0), (True, 5e-5)):
                            ph = one_photon(incoming(0.4), [0.0, 1.0, 0.0], wavelength=350.0 + 25.0 * (ncalls % 7), weight=weight)
                            end, after, command = both_single(
                                ref, packed, 'propagate_to_boundary', ph,
                                '%d components, absorption %g, scattering %g, distance %g, scatter_first %d, weights %s (%g)' % (
                                    ncomp, absorption, scattering, distance, scatter_first, use_weights, weight),
                                seed=2, photon_id=ncalls, n1=1.5, n2=1.0, absorption_length=absorption, scattering_length=scattering,
                                material1=material, distance_to_boundary=distance, use_weights=use_weights, scatter_first=scatter_first)
                            assert after >= 2
                            commands.add(command)
                            flags |= int(end.flags[0])
                            ncalls += 1
    assert ncalls == 486 and commands == {BREAK, CONTINUE, PASS}
    assert flags & (event.BULK_ABSORB | event.BULK_REEMIT | event.RAYLEIGH_SCATTER) == event.BULK_ABSORB | event.BULK_REEMIT | event.RAYLEIGH_SCATTER


def test_propagate_at_surface_edges(ref):
    """Every surface model at its parameter edges: a film of no thickness and one so thick that exp overflows (NaN
    probabilities from there on), transmissive on and off; WLS that never and that always re-emits; dichroic incidence below
    the first table angle, at a table angle, above the last, and a table of ONE angle; the default model.  With and without
    weights (alive, and below the threshold)."""
    geometry, packed = world('single')
    names = ['film_blind', 'default_blind', 'film0', 'film_thick', 'film_opaque', 'film', 'wls_never', 'wls_always', 'dichroic1', 'dichroic5', 'dichroic0', 'default']
    surfaces = {name: _index(geometry.unique_surfaces, name) for name in names}
    a = packed.arrays
    assert [int(a['surf_model'][surfaces[n]]) for n in names] == [1, 0, 1, 1, 1, 1, 2, 2, 3, 3, 3, 0]
    assert a['surf_thickness'][surfaces['film0']] == 0.0 and a['surf_transmissive'][surfaces['film_opaque']] == 0
    one = int(a['surf_dichroic_index'][surfaces['dichroic1']])
    assert a['dichroic_nangles'][one] == 1
    # (the reference reads the row BEHIND a one-angle table, weighted by zero: keep that row inside the table)
    assert a['dichroic_offset'][one] + 1 < len(a['dichroic_angles'])
    angles = [0.0, 0.1, 0.2, 0.5, float(np.arccos(np.float32(0.5))), 1.25, 1.4, np.pi / 2 - 1e-4]
    directions = [incoming(t) for t in angles]
    directions[4] = np.array([np.sqrt(0.75), 0.0, -0.5], dtype=np.float32)        # dot(normal, -direction) = 0.5 exactly
    ncalls = 0
    seen, weighted = {}, {}
    for name in names:
        for k, direction in enumerate(directions):
            s, p = s_and_p(direction)
            for pol in (s, p, (s + p) / np.sqrt(2.0)):
                for use_weights, weight in ((False, 1.0), (True, 1.0), (True, 5e-5)):
                    for wavelength in (350.0, 450.0):
                        ph = one_photon(direction, pol, wavelength=wavelength, weight=weight)
                        end, after, command = both_single(
                            ref, packed, 'propagate_at_surface', ph,
                            '%s, incidence %g, weights %s (%g), %g nm' % (name, angles[k], use_weights, weight, wavelength),
                            seed=4, photon_id=ncalls, normal=Z, n1=1.5, n2=1.0, surface_index=surfaces[name], use_weights=use_weights)
                        seen.setdefault(name, set()).add((command, int(end.flags[0])))
                        if use_weights and weight == 1.0:
                            weighted.setdefault(name, set()).add((command, int(end.flags[0])))
                        ncalls += 1
    assert ncalls == len(names) * 8 * 3 * 3 * 2
    assert any(f & event.SURFACE_REEMIT for _, f in seen['wls_always']) and not any(f & event.SURFACE_REEMIT for _, f in seen['wls_never'])
    assert any(f & event.SURFACE_TRANSMIT for _, f in seen['film']) and not any(f & event.SURFACE_TRANSMIT for _, f in seen['film_opaque'])
    for name in ('dichroic1', 'dichroic5', 'dichroic0'):
        assert {c for c, _ in seen[name]} == {BREAK, CONTINUE, PASS}, name
    assert {c for c, _ in seen['default']} >= {BREAK, CONTINUE}
    # weighted, living photons on the surfaces that detect nothing: some are reflected and some pass, by the rescaled probabilities
    for name, passing in (('film_blind', CONTINUE), ('default_blind', PASS)):
        assert any(f & (event.REFLECT_SPECULAR | event.REFLECT_DIFFUSE) for _, f in weighted[name]), name
        assert any(c == passing and not f & (event.REFLECT_SPECULAR | event.REFLECT_DIFFUSE) for c, f in weighted[name]), name


# ---- the DAQ -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def daq_input():
    """The setup of test_gpu_parity.test_daq_matches_oracle_and_reference_test: 60000 bomb photons at t = 100 ns on
    demo.tiny(), propagated to the end (here by the oracle), and the detector's CDF tables."""
    import oracle
    from chroma_amd.gpu.daq import _padded_cdf
    geometry, packed = world('tiny')
    ph = oracle.generate_bomb(60000, seed=31)
    ph.t[:] = 100.0
    end, _, _ = oracle.propagate(packed, ph, seed=9, max_steps=100, nthreads=4)
    # (non-negative charge tables only: daq.cu's own float -> unsigned conversion, compiled for the host, is undefined below zero)
    tables = _padded_cdf(*geometry.time_cdf) + _padded_cdf(*geometry.charge_cdf)
    unit = float(np.float32(geometry.charge_cdf[0][-1] / 2 ** 16))
    rng = np.random.default_rng(5)
    end.weights[:] = rng.uniform(0.2, 1.0, len(end)).astype(np.float32)     # (so that the weight gate decides)
    end.weights[::5] = 1.0
    return packed, end, tables, unit


def _daq_both(ref, many, what, states=None, **kw):
    packed, end, tables, unit = daq_input()
    out = {}
    for variant in VARIANTS:
        results = []
        for reference in (False, True):
            nwords = packed.desc.nchannels if not many else kw['ndaq'] * kw.get('channel_stride', packed.desc.nchannels)
            state = ref.daq_state(nwords) if states is None else tuple(a.copy() for a in states[variant])
            fn = ref.run_daq_many if many else ref.run_daq
            fn(packed, end, tables, unit, seed=9, variant=variant, reference=reference, state=state, **kw)
            results.append(state)
        for name, a, b in zip(('earliest_time_int', 'channel_q_int', 'channel_histories'), results[1], results[0]):
            assert np.array_equal(a, b), '%s, %s, %s: %d channels differ' % (what, variant, name, np.count_nonzero(a != b))
        out[variant] = results[0]
    return out


@pytest.mark.parametrize('acquisition', [0, 2])
@pytest.mark.parametrize('weight', [1.0, 0.3])
def test_run_daq(ref, weight, acquisition):
    first = _daq_both(ref, False, 'run_daq, weight %g, acquisition %d' % (weight, acquisition), weight=weight, acquisition=acquisition)
    t = first['contract'][0].view(np.float32)
    assert np.count_nonzero(t < 1e8) > 10
    # a second acquire onto the same state, without a reset
    second = _daq_both(ref, False, 'run_daq, second acquire', states=first, weight=weight, acquisition=acquisition + 1)
    assert (second['contract'][1] >= first['contract'][1]).all() and second['contract'][1].sum() > first['contract'][1].sum()
    assert (second['contract'][0] <= first['contract'][0]).all()


@pytest.mark.parametrize('ndaq', [1, 7, 64])
def test_run_daq_many(ref, ndaq):
    packed = daq_input()[0]
    nchannels = packed.desc.nchannels
    for weight, acquisition, stride in ((1.0, 0, nchannels), (0.3, 2, nchannels), (0.3, 0, nchannels + 3)):
        what = 'run_daq_many, %d copies, weight %g, acquisition %d, stride %d' % (ndaq, weight, acquisition, stride)
        first = _daq_both(ref, True, what, ndaq=ndaq, weight=weight, acquisition=acquisition, channel_stride=stride)
        t, q, hist = first['contract']
        hit = t.view(np.float32) < 1e8
        assert hit.reshape(ndaq, stride)[:, :nchannels].sum(axis=1).min() > 10
        if stride > nchannels:                                                  # the words between the copies stay as reset
            gap = np.ones(ndaq * stride, dtype=bool).reshape(ndaq, stride); gap[:, :nchannels] = False
            assert not hit[gap.ravel()].any() and not q[gap.ravel()].any() and not hist[gap.ravel()].any()
    second = _daq_both(ref, True, 'run_daq_many, second acquire', states=first, ndaq=ndaq, weight=0.3, acquisition=1, channel_stride=nchannels + 3)
    assert second['contract'][1].sum() > first['contract'][1].sum()
