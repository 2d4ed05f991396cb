"""The charged-particle stepper on the host: the stopping-power tables against a float64 restatement of their formulas, the
one-medium tracks of chroma_particles_track_host, the edges of one iteration through chroma_particles_advance_host, and the
tracks' segments through the light source.  No GPU."""
import numpy as np
import pytest

from chroma_amd import event
from chroma_amd.demo.optics import water
from chroma_amd.geometry import Material
from chroma_amd.generator import particles as P
from chroma_amd.generator import steps as S

f32 = np.float32
ME, K = 0.51099895, 0.307075
MASS = {1: 105.6583755, 2: 139.57039, 3: 493.677, 4: 938.27208816, 5: 3727.3794066}
CHARGE = {1: 1.0, 2: 1.0, 3: 1.0, 4: 1.0, 5: 2.0}
STOPPED, LEFT, TRUNCATED, UNTRACKED, NAN_ABORT = (P.STATUS[k] for k in ('STOPPED', 'LEFT', 'TRUNCATED', 'UNTRACKED', 'NAN_ABORT'))


def vertex(name, ke, direction=(0, 0, 1), pos=(0, 0, 0), t0=0.0):
    return event.Vertex(name, pos, direction, ke, t0=t0, pdgcode=P.PDG_CODES.get(name))


@pytest.fixture(scope='module')
def media():
    return P.StoppingMedia([water])


# ---- tables ------------------------------------------------------------------------------------------------------------
def expected_rows(material, ke):
    """The rows of ``material`` at the nodes ``ke`` and its X0 (mm), from the formulas as the issue states them, in float64."""
    elements = {'H': (1, 1.008), 'O': (8, 15.999)}
    rho = material.density
    zoa = sum(w * elements[s][0] / elements[s][1] for s, w in material.composition.items())
    def excitation(z):
        return 19.2 if z == 1 else (12.0 * z + 7.0 if z < 13 else 9.76 * z + 58.8 * z ** -0.19)
    ln_i = sum(w * elements[s][0] / elements[s][1] * np.log(excitation(elements[s][0])) for s, w in material.composition.items()) / zoa
    I = np.exp(ln_i) * 1e-6
    inv_x0 = rho * sum(w / (716.4 * elements[s][1] / (elements[s][0] * (elements[s][0] + 1) * np.log(287 / np.sqrt(elements[s][0]))))
                       for s, w in material.composition.items())          # 1/cm
    x0 = 10.0 / inv_x0

    def under_peak(s):
        peak = np.argmax(s)
        s = s.copy()
        s[:peak] = s[peak] * np.sqrt(ke[:peak] / ke[peak])
        return s
    rows = np.zeros((6, len(ke)))
    tau = ke / ME
    beta2 = 1 - 1 / (1 + tau) ** 2
    collision = 0.5 * K * zoa * rho / beta2 * (np.log(tau ** 2 * (tau + 2) / (2 * (I / ME) ** 2)) + 1 - beta2 +
                                               (tau ** 2 / 8 - (2 * tau + 1) * np.log(2)) / (tau + 1) ** 2)
    rows[0] = under_peak(collision / 10.0) + (ke + ME) / x0
    for row, M in MASS.items():
        gamma = 1 + ke / M
        beta2 = 1 - 1 / gamma ** 2
        bg2 = beta2 * gamma ** 2
        tmax = 2 * ME * bg2 / (1 + 2 * gamma * ME / M + (ME / M) ** 2)
        rows[row] = under_peak(K * CHARGE[row] ** 2 * zoa * rho / beta2 * (0.5 * np.log(2 * ME * bg2 * tmax / I ** 2) - beta2) / 10.0)
    return rows, x0


def test_tables_are_the_formulas_at_every_node(media):
    assert media.nodes == 513 and media.ke[0] == pytest.approx(1e-3) and media.ke[-1] == pytest.approx(1e5)
    want, x0 = expected_rows(water, media.ke)
    assert (want > 0).all()
    np.testing.assert_allclose(media.stopping_power[0], want, rtol=1e-6)
    assert media.radiation_length[0] == pytest.approx(x0, rel=1e-6)
    assert media.birks[0] == 0 and media.stopping_power.dtype == np.float32


def test_water_against_the_particle_data_group(media):
    muon = media.stopping_power[0, 1].astype(np.float64) * 10.0 / water.density          # MeV cm^2 / g
    assert abs(muon.min() / 1.992 - 1) < 0.08
    assert 100 < media.ke[np.argmin(muon)] < 1000          # (minimum ionisation: beta gamma of 3 to 4)
    assert abs(media.radiation_length[0] / 360.8 - 1) < 0.05


def test_unknown_element_vacuum_overrides_and_refusals():
    bad = Material('bad')
    bad.density, bad.composition = 1.0, {'Uuo': 1.0}
    with pytest.raises(ValueError, match='unknown element'):
        P.StoppingMedia([bad])
    vacuum, no_composition = Material('vacuum'), Material('dense_nothing')
    no_composition.density = 2.0
    media = P.StoppingMedia([water, vacuum, no_composition], birks={'water': 0.126}, excitation_energy={'water': 79.7})
    assert not media.stopping_power[1:].any() and np.isinf(media.radiation_length[1:]).all()
    assert media.birks[0] == f32(0.126) and media.excitation_energy[0] == 79.7
    assert (media.stopping_power[0, 1:] < P.StoppingMedia([water]).stopping_power[0, 1:]).any()          # (a larger I: less loss)
    for symbol in ('H', 'He', 'C', 'N', 'O', 'F', 'Na', 'Al', 'Si', 'Ar', 'Ca', 'Fe', 'Cu', 'Xe'):
        assert symbol in P.ELEMENTS
    with pytest.raises(ValueError):
        P.StoppingMedia([water], birks={'water': -1.0})
    with pytest.raises(ValueError):
        P.StoppingMedia([water], birks={'water': float('nan')})
    with pytest.raises(ValueError):
        P.StoppingMedia([])


# ---- one-medium tracks -------------------------------------------------------------------------------------------------
KINDS = [('mu-', 100.0), ('e-', 10.0), ('p', 50.0), ('alpha', 20.0)]


def ulp(x):
    return np.spacing(np.abs(x).astype(f32))


@pytest.mark.parametrize('scatter', [False, True])
def test_tracks_keep_the_step_rules(media, scatter):
    stepper = P.Stepper(media, max_steps=400, max_step=5.0, max_loss=0.05, ke_cut=0.05, scatter=scatter)
    vertices = [vertex(name, ke, direction=(1, 2, 2), pos=(1, 2, 3), t0=5.0) for name, ke in KINDS]
    stepped, tracks = P.track(vertices, stepper, seed=3)
    assert len(tracks) == 4 and (tracks.status == STOPPED).all()
    for i, (v, (name, ke0)) in enumerate(zip(stepped, KINDS)):
        s = v.steps
        assert v is not vertices[i] and vertices[i].steps is None
        lo, hi = int(tracks.offsets[i]), int(tracks.offsets[i + 1])
        assert len(s.x) == hi - lo and 10 < len(s.x) <= 401
        # point 0: the vertex, nothing deposited
        assert (s.x[0], s.y[0], s.z[0], s.t[0], s.ke[0], s.edep[0], s.qedep[0]) == (1, 2, 3, 5, f32(ke0), 0, 0)
        np.testing.assert_allclose([s.dx[0], s.dy[0], s.dz[0]], [1 / 3, 2 / 3, 2 / 3], rtol=1e-6)
        assert tracks.medium[lo] == -1 and (tracks.medium[lo + 1:hi] == 0).all()
        assert all(a.dtype == np.float32 for a in (s.x, s.t, s.ke, s.edep, s.qedep))
        # the energy book-keeping is exact, and a stopped track has deposited everything
        assert np.array_equal(s.ke[1:], s.ke[:-1] - s.edep[1:])
        assert s.ke[-1] == 0 and (s.ke[:-1] >= f32(0.05)).all()
        assert np.array_equal(s.qedep, s.edep)          # (no Birks constant)
        length = np.sqrt(np.diff(s.x.astype(np.float64)) ** 2 + np.diff(s.y.astype(np.float64)) ** 2 + np.diff(s.z.astype(np.float64)) ** 2)
        # (measured between rounded positions: each end is off by half an ulp of its largest coordinate per axis, and |dir| by 1e-6)
        reach = np.maximum(np.abs(tracks.pos[lo:hi - 1]).max(axis=1), np.abs(tracks.pos[lo + 1:hi]).max(axis=1))
        assert (length <= 5.0 * (1 + 1e-6) + 2 * ulp(reach)).all()
        assert (s.edep[1:-1] <= f32(0.05) * s.ke[:-2] + ulp(s.ke[:-2])).all()
        assert (np.diff(s.t) > 0).all()
        assert (np.abs(np.sqrt(s.dx.astype(np.float64) ** 2 + s.dy.astype(np.float64) ** 2 + s.dz.astype(np.float64) ** 2) - 1) < 1e-6).all()
        if not scatter:
            assert np.array_equal(s.dx, np.full_like(s.dx, s.dx[0]))


@pytest.mark.parametrize('name,ke0', KINDS)
def test_path_length_is_the_csda_range(media, name, ke0):
    stepper = P.Stepper(media, max_steps=2000, max_step=1e6, max_loss=0.01, ke_cut=0.05, scatter=False)
    stepped, tracks = P.track([vertex(name, ke0)], stepper, seed=1)
    s = stepped[0].steps
    assert tracks.status[0] == STOPPED
    row = P.SPECIES[abs(P.PDG_CODES[name])]
    ke = np.exp(np.linspace(np.log(0.05), np.log(ke0), 20001))
    integrand = 1.0 / media.interpolate(0, row, ke)
    csda = float((0.5 * (integrand[1:] + integrand[:-1]) * np.diff(ke)).sum())
    print('%s %g MeV: path %.6g mm, CSDA range %.6g mm, ratio %.5f, %d steps' % (name, ke0, s.z[-1], csda, s.z[-1] / csda, len(s.x) - 1))
    assert abs(float(s.z[-1]) / csda - 1) < 0.02
    # collinear with (0, 0, 1), and forward (the last steps of a long track are shorter than an ulp of its position)
    assert not s.x.any() and not s.y.any() and (np.diff(s.z) >= 0).all() and (np.diff(s.z)[:50] > 0).all()


def test_highland_width(media):
    n = 4096
    x0 = float(media.radiation_length[0])
    stepper = P.Stepper(media, max_steps=1, max_step=0.01 * x0, max_loss=1.0, ke_cut=0.0, scatter=True)
    stepped, tracks = P.track([vertex('mu-', 1000.0)] * n, stepper, seed=11)
    assert (tracks.status == TRUNCATED).all() and np.array_equal(np.diff(tracks.offsets), np.full(n, 2))
    d = tracks.dir[1::2].astype(np.float64)
    theta_x, theta_y = np.arctan2(d[:, 0], d[:, 2]), np.arctan2(d[:, 1], d[:, 2])
    M = MASS[1]
    p = np.sqrt(1000.0 * (1000.0 + 2 * M))
    beta = p / (1000.0 + M)
    step = float(f32(0.01 * x0))
    theta0 = 13.6 / (beta * p) * np.sqrt(step / x0) * (1 + 0.038 * np.log(step / (x0 * beta ** 2)))
    for theta in (theta_x, theta_y):
        rms = np.sqrt((theta ** 2).mean())
        print('rms %.6g, theta0 %.6g, ratio %.4f' % (rms, theta0, rms / theta0))
        assert abs(rms / theta0 - 1) < 0.05
    assert abs(np.corrcoef(theta_x, theta_y)[0, 1]) < 0.08          # (5 sigma of 1/sqrt(n))


def flat(tracks):
    return [getattr(tracks, name) for name in ('pos', 't', 'dir', 'ke', 'edep', 'qedep', 'medium')]


def test_tracks_do_not_depend_on_the_split_into_calls(media):
    stepper = P.Stepper(media, max_steps=300, max_step=5.0)
    vertices = [vertex(name, ke, direction=(1, k, 2)) for k, (name, ke) in enumerate(KINDS + KINDS[:2])]
    _, whole = P.track(vertices, stepper, seed=7, particle_base=10)
    _, head = P.track(vertices[:2], stepper, seed=7, particle_base=10)
    _, tail = P.track(vertices[2:], stepper, seed=7, particle_base=12)
    for w, h, t in zip(flat(whole), flat(head), flat(tail)):
        assert np.array_equal(w, np.concatenate([h, t]))
    assert np.array_equal(whole.offsets, np.concatenate([head.offsets, tail.offsets[1:] + head.offsets[-1]]))
    _, other = P.track(vertices, stepper, seed=8, particle_base=10)
    assert not np.array_equal(whole.dir[:len(other.dir)], other.dir[:len(whole.dir)])
    _, shifted = P.track(vertices, stepper, seed=7, particle_base=11)
    assert not np.array_equal(whole.dir[:len(shifted.dir)], shifted.dir[:len(whole.dir)])


# ---- the edges of one iteration ----------------------------------------------------------------------------------------
class One(object):
    """One particle and its matrix, advanced through chroma_particles_advance_host"""

    def __init__(self, media, name='mu-', ke=100.0, pos=(0, 0, 0), **stepper):
        options = dict(max_steps=4, max_step=5.0, max_loss=0.05, ke_cut=0.05, scatter=False, outside=0)
        options.update(stepper)
        self.stepper = P.Stepper(media, **options)
        self.state = P.ParticleState([vertex(name, ke, pos=pos)])
        self.matrix, self.struct = P.point_arrays(self.stepper.max_steps + 1, fill=-7)

    def advance(self, distance=None, triangle=None, medium=None, seed=1):
        wrap = lambda x: None if x is None else [x]
        P.advance(self.state, self.stepper, seed, self.struct, wrap(distance), wrap(triangle), wrap(medium))
        return self

    @property
    def status(self):
        return int(self.state.status[0])

    def rows_written(self):
        return int((self.matrix['medium'] != -7).sum())


@pytest.fixture(scope='module')
def two_media():
    return P.StoppingMedia([water, Material('vacuum')])


def test_edge_boundary_at_zero_and_at_the_physics_step(two_media):
    at_zero = One(two_media).advance(distance=0.0, triangle=7, medium=0)
    assert at_zero.status == 0 and at_zero.state.nsteps[0] == 1 and at_zero.state.last_hit[0] == 7
    assert at_zero.rows_written() == 2 and not at_zero.matrix['pos'][1].any() and at_zero.matrix['edep'][1] == 0
    assert at_zero.matrix['ke'][1] == 100 and at_zero.matrix['t'][1] == 0 and at_zero.matrix['medium'][1] == 0
    free = One(two_media).advance()          # nothing ahead, in the `outside` row: the physics step
    s_phys = free.matrix['pos'][1, 2]
    assert free.status == 0 and free.state.last_hit[0] == -1 and 0 < s_phys <= 5.0 and free.matrix['medium'][1] == 0
    exact = One(two_media).advance(distance=s_phys, triangle=3, medium=0)
    assert exact.state.last_hit[0] == 3 and exact.matrix['pos'][1, 2] == s_phys
    beyond = One(two_media).advance(distance=np.nextafter(s_phys, f32(np.inf)), triangle=3, medium=0)
    assert beyond.state.last_hit[0] == -1 and beyond.matrix['pos'][1, 2] == s_phys
    for name in ('ke', 'edep', 't'):
        assert exact.matrix[name][1] == free.matrix[name][1] == beyond.matrix[name][1]
    no_triangle = One(two_media).advance(distance=1.0, triangle=-1, medium=0)          # a distance without a triangle is no hit
    assert no_triangle.matrix['pos'][1, 2] == s_phys


def test_edge_leaving(two_media):
    in_vacuum = One(two_media).advance(distance=np.inf, triangle=-1, medium=1)
    assert in_vacuum.status == LEFT and in_vacuum.rows_written() == 1 and in_vacuum.state.nsteps[0] == 0
    assert in_vacuum.matrix['medium'][0] == -1 and in_vacuum.matrix['ke'][0] == 100
    through_vacuum = One(two_media).advance(distance=3.0, triangle=5, medium=1)          # a triangle ahead: a free flight to it
    assert through_vacuum.status == 0 and through_vacuum.matrix['pos'][1, 2] == 3 and through_vacuum.matrix['edep'][1] == 0
    assert through_vacuum.matrix['ke'][1] == 100 and through_vacuum.state.last_hit[0] == 5 and through_vacuum.matrix['t'][1] > 0
    for medium in (-1, 2, 1000):
        gone = One(two_media).advance(distance=1.0, triangle=0, medium=medium)
        assert gone.status == LEFT and gone.rows_written() == 1
    no_outside = One(two_media, outside=-1).advance()
    assert no_outside.status == LEFT and no_outside.rows_written() == 1
    again = no_outside.advance()          # a particle that is not alive is not touched
    assert again.status == LEFT and again.rows_written() == 1


def test_edge_the_energy_cut(two_media):
    probe = One(two_media, name='p', ke=1.0).advance()
    ke1 = probe.matrix['ke'][1]
    assert 0 < ke1 < 1 and probe.status == 0
    above = One(two_media, name='p', ke=1.0, ke_cut=float(ke1)).advance()
    assert above.status == 0 and above.matrix['ke'][1] == ke1 and above.matrix['edep'][1] == probe.matrix['edep'][1]
    below = One(two_media, name='p', ke=1.0, ke_cut=float(np.nextafter(ke1, f32(2)))).advance()
    assert below.status == STOPPED and below.matrix['ke'][1] == 0 and below.matrix['edep'][1] == 1
    assert below.matrix['pos'][1, 2] == probe.matrix['pos'][1, 2] and below.state.ke[0] == 0


def test_edge_untracked_truncated_and_nan(two_media):
    unknown = One(two_media, name='gamma', ke=1.0).advance(distance=1.0, triangle=0, medium=0)
    assert unknown.state.species[0] == -1 and unknown.status == UNTRACKED and unknown.rows_written() == 1 and unknown.state.nsteps[0] == 0
    at_rest = One(two_media, ke=0.0).advance()
    assert at_rest.status == UNTRACKED and at_rest.rows_written() == 1
    short = One(two_media, max_steps=2).advance()
    assert short.status == 0
    short.advance()
    assert short.status == TRUNCATED and short.state.nsteps[0] == 2 and short.rows_written() == 3
    short.advance()
    assert short.state.nsteps[0] == 2 and short.rows_written() == 3
    lost = One(two_media, pos=(0, np.nan, 0)).advance()
    assert lost.status == NAN_ABORT and lost.rows_written() == 2 and np.isnan(lost.matrix['pos'][1, 1])


# ---- through the light source ------------------------------------------------------------------------------------------
def test_segments_feed_the_light_source(media):
    light = S.LightMedia([water])
    stepper = P.Stepper(P.StoppingMedia([water], birks={'water': 0.1}), max_steps=400, max_step=5.0)
    _, tracks = P.track([vertex('mu-', 100.0), vertex('gamma', 1.0), vertex('p', 30.0)], stepper, seed=5, evidx=[4, 5, 6])
    segments, medium = tracks.segments()
    counts = np.diff(tracks.offsets.astype(np.int64))
    assert counts[1] == 1 and len(segments) == counts.sum() - 3 and len(medium) == len(segments)
    # the segments are the points: beta from the two ends' energies in single precision, deposits and medium of the end point
    lo = int(tracks.offsets[0])
    nmu = int(counts[0]) - 1
    gamma = f32(1) + tracks.ke[lo:lo + nmu + 1] / f32(MASS[1])
    beta = np.sqrt(f32(1) - f32(1) / (gamma * gamma), dtype=f32)
    assert np.array_equal(segments.beta[:nmu], f32(0.5) * (beta[:-1] + beta[1:]))
    assert np.array_equal(segments.a[:nmu], tracks.pos[lo:lo + nmu]) and np.array_equal(segments.b[:nmu], tracks.pos[lo + 1:lo + nmu + 1])
    assert np.array_equal(segments.qedep[:nmu], tracks.qedep[lo + 1:lo + nmu + 1]) and (segments.qedep[:nmu] < tracks.edep[lo + 1:lo + nmu + 1]).all()
    assert np.array_equal(segments.t_b[:nmu], tracks.t[lo + 1:lo + nmu + 1]) and (medium == 0).all()
    assert (segments.evidx[:nmu] == 4).all() and (segments.evidx[nmu:] == 6).all() and (segments.z[:nmu] == -1).all() and (segments.z[nmu:] == 1).all()
    offsets, total = S.count_photons(segments, light, seed=9, medium=medium)
    cherenkov = (offsets[1::2] - offsets[0:-1:2]).astype(np.int64)
    source = light.sources[0]
    n_max = float(source.refractive_index[source.cherenkov_nodes[0]:source.cherenkov_nodes[1] + 1].max())
    assert cherenkov[:5].min() > 0          # a 100 MeV muon is above threshold (beta 0.86 against 1/n of 0.75)
    below = segments.beta < 1.0 / n_max
    assert below[:nmu].any() and below[nmu:].all() and not cherenkov[below].any()
    photons = S.generate_photons(segments, light, seed=9, medium=medium)
    assert len(photons) == total and (photons.flags[:int(offsets[1])] == event.CHERENKOV).all()
    assert set(np.unique(photons.evidx)) <= {4, 6}
