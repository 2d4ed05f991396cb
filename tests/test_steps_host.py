"""Photons from charged-particle steps, host twin (chroma_steps_count_host / chroma_steps_generate_host) against a NumPy
restatement written here: its own Philox4x32-10, cm_u32_to_uniform's mapping (exact in float32), the counting rules, the
Cherenkov photon in float32 NumPy, and the closed forms and distributions the photons have to follow.  No GPU."""
import numpy as np
import pytest

from chroma_amd import event
from chroma_amd.generator import steps
from chroma_amd.geometry import Material, standard_wavelengths

f32 = np.float32
EPS = float(np.finfo(np.float32).eps)
ALPHA = 7.2973525693e-3
SEED = 0x1234567887654321
M32 = 0xFFFFFFFF


# ---- the restatement ---------------------------------------------------------------------------------------------------
def philox(c, k):
    """Philox4x32-10 (Salmon et al., SC'11) on Python integers."""
    c0, c1, c2, c3 = c
    k0, k1 = k
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


class Stream(object):
    """Draw k of (seed, id, stream word): word k & 3 of block k >> 2, counter = (block, word, id lo, id hi)."""

    def __init__(self, seed, ident, word):
        self.key = (seed & M32, seed >> 32)
        self.ident, self.word, self.k, self.block = int(ident), int(word), 0, None

    def uniform(self):
        if self.block is None or self.k >> 2 != self.block[0]:
            b = self.k >> 2
            self.block = (b, philox((b, self.word, self.ident & M32, self.ident >> 32), self.key))
        x = self.block[1][self.k & 3]
        self.k += 1
        return f32(x) * f32(2.3283064365386963e-10) + f32(1.1641532182693481e-10)


def segment_id(g):
    return 0x57E9000000000000 + g


class Margin(object):
    """The closest a Knuth product came to its threshold (relative): the test's threshold is exp() in double precision,
    the library's a float32 polynomial, and a decision is theirs in common only away from it."""
    closest = np.inf


def draw_count(stream, mean):
    if not mean > 0:
        return 0
    if mean <= 16:
        limit, p, k = np.exp(-np.float64(mean)), f32(1), 0
        while True:
            p = p * stream.uniform()
            k += 1
            Margin.closest = min(Margin.closest, abs(float(p) / limit - 1.0))
            if not p > limit:
                return k - 1
    u1, u2 = stream.uniform(), stream.uniform()
    normal = np.sqrt(-2.0 * np.log(np.float64(u1))) * np.cos(np.float64(f32(6.2831855) * u2))
    return max(0, int(np.floor(float(mean) + np.sqrt(float(mean)) * normal + 0.5)))


def cherenkov_mean32(src, L, beta, z):
    """The mean as the library forms it: float32, in its order."""
    L, beta, z = f32(L), f32(beta), f32(z)
    if not (L > 0 and beta > 0 and z != 0):
        return f32(0)
    s = src.struct
    lo, hi = src.cherenkov_nodes
    beta2, total, prev = beta * beta, f32(0), f32(0)
    for j in range(lo, hi + 1):
        wl = f32(s.wavelength_start) + f32(j) * f32(s.wavelength_step)
        n = src.refractive_index[j]
        f = f32(1) - f32(1) / (beta2 * (n * n))
        f = f / (wl * wl) if f > 0 else f32(0)
        if j > lo:
            total = total + f32(0.5) * (prev + f) * f32(s.wavelength_step)
        prev = f
    return ((f32(45850.6183) * (z * z)) * L) * total


def interp32(src, x, table):
    s = src.struct
    start, step, n = f32(s.wavelength_start), f32(s.wavelength_step), s.wavelength_n
    if x < start:
        return table[0]
    if x > start + f32(n - 1) * step:
        return table[n - 1]
    jl = int((x - start) / step)
    ju = min(jl + 1, n - 1)
    return table[jl] + (x - (start + f32(jl) * step)) * (table[ju] - table[jl]) / step


def dot32(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def cross32(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], dtype=f32)


def cherenkov_photon32(src, seg, k, g, j):
    """Cherenkov photon j of segment k (global index g) in float32 NumPy: (pos, dir, pol, wavelength, t)."""
    r = Stream(SEED, segment_id(g), 1 + j)
    a, b = seg.a[k], seg.b[k]
    ab = b - a
    u = ab / np.sqrt(dot32(ab, ab))
    beta = seg.beta[k]
    beta2 = beta * beta
    lo, hi = src.cherenkov_nodes
    n_max = src.refractive_index[lo:hi + 1].max()
    f_max = f32(1) - f32(1) / (beta2 * (n_max * n_max))
    inv_lo, inv_hi = f32(1) / f32(src.wl_hi), f32(1) / f32(src.wl_lo)
    for _ in range(1000):
        wl = f32(1) / (inv_lo + r.uniform() * (inv_hi - inv_lo))
        n = interp32(src, wl, src.refractive_index)
        if r.uniform() * f_max <= f32(1) - f32(1) / (beta2 * (n * n)):
            break
    ct = min(f32(1) / (beta * n), f32(1))
    st = np.sqrt(f32(1) - ct * ct)
    phi = f32(0) + r.uniform() * (f32(2) * f32(np.pi) - f32(0))
    au = np.abs(u)
    axis = np.eye(3, dtype=f32)[0 if (au[0] <= au[1] and au[0] <= au[2]) else 1 if au[1] <= au[2] else 2]
    e = cross32(u, axis)
    e = e / np.sqrt(dot32(e, e))

    def rot(v):
        c, s = f32(np.cos(np.float64(phi))), f32(np.sin(np.float64(phi)))
        return (v * c + (u * dot32(v, u)) * (f32(1) - c)) + cross32(v, u) * s
    d, p = rot(u * ct + e * st), rot(u * st - e * ct)
    frac = r.uniform()
    return a + ab * frac, d, p, wl, seg.t_a[k] + frac * (seg.t_b[k] - seg.t_a[k])


def chi2_ok(observed, expected):
    """Pearson's chi-squared of the counts against the expected counts (bins expecting fewer than 20 lumped into one) within
    5 sigma of its mean: dof + 5 sqrt(2 dof)."""
    observed, expected = np.asarray(observed, dtype=np.float64), np.asarray(expected, dtype=np.float64)
    assert abs(observed.sum() - expected.sum()) < 1e-6 * expected.sum() + 1e-9
    small = expected < 20
    if small.any():
        observed = np.append(observed[~small], observed[small].sum())
        expected = np.append(expected[~small], expected[small].sum())
        if expected[-1] < 5:                 # (too few even together: into the largest bin)
            k = int(np.argmax(expected[:-1]))
            observed[k] += observed[-1]; expected[k] += expected[-1]
            observed, expected = observed[:-1], expected[:-1]
    dof = len(expected) - 1
    chi2 = ((observed - expected) ** 2 / expected).sum()
    print('chi2 %.1f, dof %d, bound %.1f' % (chi2, dof, dof + 5 * np.sqrt(2 * dof)))
    return chi2 <= dof + 5 * np.sqrt(2 * dof)


# ---- media and segments ------------------------------------------------------------------------------------------------
WL = standard_wavelengths.astype(np.float64)
TIMES = np.arange(0, 1000, 0.05)


def medium(n=1.5, spectrum=False, light_yield=None, waveform=False):
    m = Material('medium')
    m.set('refractive_index', n)
    if spectrum:
        m.set('scintillation_spectrum', np.where(np.abs(WL - 430) < 50, 1.0 + np.cos((WL - 430) * np.pi / 50), 0.0))
        m.scintillation_light_yield = light_yield
    if waveform:
        t = TIMES
        m.scintillation_waveform = np.column_stack([t, 0.7 * np.exp(-t / 3.0) / 3.0 + 0.3 * np.exp(-t / 12.0) / 12.0])
    return m


SLOPED_N = 1.38 - (WL - 200.0) * 1e-4              # 1.38 at 200 nm, 1.32 at 800 nm


def track(n, a=(0, 0, 0), b=(100, 0, 0), t=(0.0, 0.4), beta=0.9, z=1.0, qedep=0.0, evidx=0):
    """n segments cut from the straight line a -> b."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    x = a + (b - a) * np.linspace(0, 1, n + 1)[:, None]
    tt = np.linspace(t[0], t[1], n + 1)
    return steps.Segments(x[:-1], x[1:], tt[:-1], tt[1:], beta, z, qedep, evidx)


def identical(n, length=1.0, beta=0.9, z=1.0, qedep=0.0, direction=(1, 2, 2), t=(0.0, 0.0)):
    d = np.asarray(direction, dtype=np.float64)
    d = d / np.linalg.norm(d)
    a = np.tile(np.array([10.0, -20.0, 30.0]), (n, 1))
    return steps.Segments(a, a + length * d, t[0], t[1], beta, z, qedep, 0)


def counts_of(seg, src, seed=SEED):
    offsets, total = steps.count_photons(seg, src, seed)
    c = np.diff(offsets.astype(np.int64))
    assert total == offsets[-1] and offsets[0] == 0
    return c[0::2], c[1::2]


# ---- counts ------------------------------------------------------------------------------------------------------------
def test_counts_are_those_of_the_restatement_bit_for_bit():
    src = steps.LightSource(medium(SLOPED_N, spectrum=True, light_yield=10.0), WL)
    rng = np.random.default_rng(5)
    n = 300
    # Cherenkov means 0 .. ~12 (lengths 0 .. 0.06 mm at ~200 photons / mm), scintillation means 0 .. 15; some of either zero
    length = rng.uniform(0, 0.06, n) * (rng.uniform(size=n) > 0.1)
    qedep = rng.uniform(0, 1.5, n).astype(f32) * (rng.uniform(size=n) > 0.1)
    a = rng.uniform(-50, 50, (n, 3))
    seg = steps.Segments(a, a + length[:, None] * np.array([0.6, 0.0, 0.8]), 0.0, 1.0, rng.uniform(0.8, 1.0, n), 1.0, qedep, 0, segment_base=1000)
    got_ch, got_sc = counts_of(seg, src)
    Margin.closest = np.inf
    want_ch, want_sc = [], []
    for k in range(n):
        r = Stream(SEED, segment_id(1000 + k), 0)
        L = np.sqrt(dot32(seg.b[k] - seg.a[k], seg.b[k] - seg.a[k]))
        mean_ch, mean_sc = cherenkov_mean32(src, L, seg.beta[k], seg.z[k]), f32(src.light_yield) * seg.qedep[k]
        assert mean_ch <= 16 and mean_sc <= 16
        want_ch.append(draw_count(r, mean_ch))
        want_sc.append(draw_count(r, mean_sc if seg.qedep[k] > 0 else 0))
    # (the decisions of this seed stay clear of the threshold: the two exponentials differ by ~1e-7 relative)
    assert Margin.closest > 1e-6
    assert np.array_equal(got_ch, want_ch) and np.array_equal(got_sc, want_sc)
    assert max(want_ch) > 5 and max(want_sc) > 10 and min(want_ch) == 0 and min(want_sc) == 0


def test_cherenkov_count_sum_follows_frank_tamm():
    n_const, beta, z, L, nseg = 1.34, 0.95, 1.0, 0.05, 2000        # ~3.3 photons a segment: the Poisson branch
    src = steps.LightSource(medium(n_const), WL, cherenkov_range=(200, 800))
    got, none = counts_of(identical(nseg, L, beta, z), src)
    assert none.sum() == 0
    lo, hi = src.wl_lo, src.wl_hi
    closed = 2 * np.pi * ALPHA * z * z * (L * 1e6) * (1 - 1 / (beta * n_const) ** 2) * (1 / lo - 1 / hi) * nseg
    wl = WL[src.cherenkov_nodes[0]:src.cherenkov_nodes[1] + 1]
    f = (1 - 1 / (beta * n_const) ** 2) / wl ** 2
    trapezoid = 2 * np.pi * ALPHA * z * z * (L * 1e6) * (0.5 * (f[1:] + f[:-1]) * np.diff(wl)).sum() * nseg
    print('photons %d, closed form %.1f, trapezoid %.1f' % (got.sum(), closed, trapezoid))
    assert abs(got.sum() - closed) <= 5 * np.sqrt(closed) + abs(trapezoid - closed)
    # the other branch (a rounded normal above a mean of 16): 0.5 mm, ~33 photons a segment
    got, _ = counts_of(identical(nseg, 10 * L, beta, z), src)
    assert abs(got.sum() - 10 * closed) <= 5 * np.sqrt(10 * closed) + 10 * abs(trapezoid - closed)
    assert closed / nseg * 10 > 16 and got.min() > 0


def test_no_cherenkov_light_below_threshold_without_charge_or_length():
    src = steps.LightSource(medium(SLOPED_N), WL)
    below = 0.999 / SLOPED_N[src.cherenkov_nodes[0]:src.cherenkov_nodes[1] + 1].max()
    for seg in (identical(50, 5.0, below), identical(50, 5.0, 0.99, z=0.0), identical(50, 0.0, 0.99)):
        ch, sc = counts_of(seg, src)
        assert ch.sum() == 0 and sc.sum() == 0
    ch, _ = counts_of(identical(50, 5.0, 0.99), src)
    assert ch.min() > 0
    # an alpha's charge counts squared
    one, _ = counts_of(identical(400, 0.5, 0.99, z=1.0), src)
    two, _ = counts_of(identical(400, 0.5, 0.99, z=-2.0), src)
    assert abs(two.sum() - 4 * one.sum()) <= 5 * np.sqrt(4 * one.sum() + 16 * one.sum())


# ---- Cherenkov photons ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def cherenkov():
    src = steps.LightSource(medium(SLOPED_N), WL)
    seg = steps.Segments.join([track(40, (0, 0, 0), (30, -40, 120), (1.0, 1.5), beta=0.8),
                               track(40, (5, 5, 5), (5, 5, -200), (2.0, 2.9), beta=0.97),
                               track(40, (-300, 10, 0), (400, 10.5, 0), (0.0, 3.0), beta=0.8)], segment_base=77)
    offsets, total = steps.count_photons(seg, src, SEED)
    photons = steps.generate_photons(seg, src, SEED)
    assert len(photons) == total and (photons.flags == event.CHERENKOV).all()
    return src, seg, offsets, photons


def test_cherenkov_photons_are_those_of_the_restatement(cherenkov):
    src, seg, offsets, p = cherenkov
    rng = np.random.default_rng(1)
    worst = 0.0
    for k in rng.choice(len(seg), 24, replace=False):
        first, n = int(offsets[2 * k]), int(offsets[2 * k + 1] - offsets[2 * k])
        for j in sorted(set([0, n - 1]) | set(rng.integers(0, n, 6).tolist())):
            pos, d, pol, wl, t = cherenkov_photon32(src, seg, k, 77 + k, j)
            i = first + j
            # the restatement takes sine and cosine from libm where the library has its own polynomials (2 ulp): 16 epsilons
            # on the unit vectors; what uses neither is equal to the last bit
            assert p.wavelengths[i] == wl and p.t[i] == t and np.array_equal(p.pos[i], pos)
            worst = max(worst, np.abs(p.dir[i] - d).max(), np.abs(p.pol[i] - pol).max())
    print('largest difference from the restatement: %.2f epsilons' % (worst / EPS))
    assert worst <= 16 * EPS
    assert (p.last_hit_triangles == -1).all() and (p.weights == 1).all() and (p.evidx == 0).all()


def test_cherenkov_cone_polarisation_position_and_time(cherenkov):
    src, seg, offsets, p = cherenkov
    owner = np.repeat(np.arange(len(seg)), np.diff(offsets.astype(np.int64))[0::2])
    a, b = seg.a[owner].astype(np.float64), seg.b[owner].astype(np.float64)
    L = np.linalg.norm(b - a, axis=1)
    u = (b - a) / L[:, None]
    d, pol = p.dir.astype(np.float64), p.pol.astype(np.float64)
    n = np.interp(p.wavelengths.astype(np.float64), WL, src.refractive_index.astype(np.float64))
    want = 1.0 / (seg.beta[owner].astype(np.float64) * n)
    # The bound: 16 float32 epsilons, unless the float32 restatement itself is further from the float64 cone on these
    # inputs -- measured here on a sample of it (it is not: ~3 epsilons).
    rng = np.random.default_rng(2)
    own = 0.0
    for i in rng.choice(len(p), 60, replace=False):
        k = owner[i]
        _, d32, _, wl32, _ = cherenkov_photon32(src, seg, k, 77 + k, int(i - offsets[2 * k]))
        n64 = np.interp(float(wl32), WL, src.refractive_index.astype(np.float64))
        own = max(own, abs(np.dot(d32.astype(np.float64), u[i]) - 1.0 / (float(seg.beta[k]) * n64)))
    bound = max(16 * EPS, own)
    print('restatement off the cone by %.2f epsilons, library by %.2f; bound %.2f'
          % (own / EPS, np.abs((d * u).sum(1) - want).max() / EPS, bound / EPS))
    assert np.abs((d * u).sum(1) - want).max() <= bound
    assert np.abs(np.linalg.norm(d, axis=1) - 1).max() <= bound and np.abs(np.linalg.norm(pol, axis=1) - 1).max() <= bound
    assert np.abs((d * pol).sum(1)).max() <= bound
    assert np.abs((pol * np.cross(u, d)).sum(1)).max() <= bound               # pol in the plane of u and dir
    assert ((pol * u).sum(1) > 0).all()
    # on the segment (distance from its line within the rounding of the coordinates), between its ends in space and time
    pos = p.pos.astype(np.float64)
    scale = np.maximum(np.abs(a).max(1), np.abs(b).max(1))
    assert (np.linalg.norm(np.cross(pos - a, u), axis=1) <= 16 * EPS * scale).all()
    along = ((pos - a) * u).sum(1)
    assert (along >= -16 * EPS * scale).all() and (along <= L + 16 * EPS * scale).all()
    assert (p.t >= seg.t_a[owner]).all() and (p.t <= seg.t_b[owner]).all()
    assert (p.wavelengths >= f32(src.wl_lo)).all() and (p.wavelengths <= f32(src.wl_hi)).all()


def test_cherenkov_spectrum_for_a_sloped_index():
    beta = 0.8
    src = steps.LightSource(medium(SLOPED_N), WL)
    p = steps.generate_photons(identical(400, 3.0, beta), src, SEED)
    assert len(p) > 30000
    edges = np.linspace(src.wl_lo, src.wl_hi, 13)
    fine = np.linspace(src.wl_lo, src.wl_hi, 120001)
    density = (1 - 1 / (beta * np.interp(fine, WL, src.refractive_index.astype(np.float64))) ** 2) / fine ** 2
    cdf = np.concatenate(([0], np.cumsum(0.5 * (density[1:] + density[:-1]))))
    share = np.diff(np.interp(edges, fine, cdf / cdf[-1]))
    assert share.max() / share.min() > 3                                     # (a shape worth testing)
    assert chi2_ok(np.histogram(p.wavelengths, edges)[0], share * len(p))


# ---- scintillation ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def scintillation():
    src = steps.LightSource(medium(1.5, spectrum=True, light_yield=100.0, waveform=True), WL)
    seg = identical(2000, 3.0, beta=0.0, z=0.0, qedep=0.073)                # mean 7.3 a segment; t_a = t_b = 0: t IS the delay
    return src, seg, steps.generate_photons(seg, src, SEED)


def test_scintillation_count_sums(scintillation):
    src, seg, p = scintillation
    expected = 100.0 * float(f32(0.073)) * len(seg)
    assert (p.flags == event.SCINTILLATION).all()
    assert abs(len(p) - expected) <= 5 * np.sqrt(expected)
    ch, sc = counts_of(identical(2000, 3.0, beta=0.0, z=0.0, qedep=0.4), src)           # mean 40: the other branch
    assert ch.sum() == 0 and abs(sc.sum() - 40.0 * 2000) <= 5 * np.sqrt(40.0 * 2000) and sc.min() > 10
    assert counts_of(identical(10, 3.0, qedep=-1.0, z=0.0), src)[1].sum() == 0
    # a medium without a spectrum or a yield does not scintillate
    assert counts_of(seg, steps.LightSource(medium(1.5), WL))[1].sum() == 0


def test_scintillation_wavelengths_and_delays_follow_their_tables(scintillation):
    src, seg, p = scintillation
    # between two grid nodes the sampled density is flat: the cells of the grid are the bins
    edges = np.append(WL, WL[-1] + 5.0) - 0.0
    assert chi2_ok(np.histogram(p.wavelengths, WL)[0], np.diff(src.scintillation_cdf.astype(np.float64)) * len(p))
    assert p.wavelengths.min() >= 380 and p.wavelengths.max() <= 480 and edges[0] == 60
    nodes = np.append(np.arange(0, 20 * 60 + 1, 20), len(TIMES) - 1)          # 1 ns bins out to 60 ns, one for the rest
    assert chi2_ok(np.histogram(p.t, TIMES[nodes])[0], np.diff(src.time_cdf.astype(np.float64)[nodes]) * len(p))
    assert p.t.min() >= 0 and p.t.max() <= TIMES[-1]
    # no waveform: prompt
    prompt = steps.generate_photons(seg[:50], steps.LightSource(medium(1.5, spectrum=True, light_yield=100.0), WL), SEED)
    assert len(prompt) and (prompt.t == 0).all()


def test_scintillation_is_isotropic_and_uniform_along_the_segment(scintillation):
    src, seg, p = scintillation
    n = len(p)
    for axis in range(3):
        assert chi2_ok(np.histogram(p.dir[:, axis], np.linspace(-1, 1, 7))[0], np.full(6, n / 6.0))
    d, pol = p.dir.astype(np.float64), p.pol.astype(np.float64)
    assert np.abs(np.linalg.norm(d, axis=1) - 1).max() <= 16 * EPS and np.abs(np.linalg.norm(pol, axis=1) - 1).max() <= 16 * EPS
    assert np.abs((d * pol).sum(1)).max() <= 16 * EPS
    a, b = seg.a[0].astype(np.float64), seg.b[0].astype(np.float64)
    frac = ((p.pos.astype(np.float64) - a) * (b - a)).sum(1) / ((b - a) ** 2).sum()
    assert frac.min() >= -1e-6 and frac.max() <= 1 + 1e-6
    assert chi2_ok(np.histogram(np.clip(frac, 0, 1), np.linspace(0, 1, 11))[0], np.full(10, n / 10.0))
    assert np.linalg.norm(np.cross(p.pos.astype(np.float64) - a, (b - a) / 3.0), axis=1).max() <= 16 * EPS * 30


# ---- vertices, batching ----------------------------------------------------------------------------------------------------
def stepped_vertex(pdgcode, n, start, direction, ke0, t0=0.0, dedx=0.2):
    x = np.asarray(start, dtype=float) + np.linspace(0, 5.0 * n, n + 1)[:, None] * np.asarray(direction, dtype=float)
    ke = ke0 - dedx * np.arange(n + 1) * 5.0
    dep = np.concatenate(([0.0], np.full(n, dedx * 5.0)))
    st = event.Steps(x[:, 0], x[:, 1], x[:, 2], t0 + np.arange(n + 1) * 5.0 / 299.79, *(np.tile(direction, (n + 1, 1)).T),
                     ke, dep, 0.8 * dep)
    return event.Vertex('particle', start, direction, ke0, t0=t0, steps=st, pdgcode=pdgcode)


def test_segments_from_vertices():
    mu, e, gamma = stepped_vertex(13, 6, (0, 0, 0), (0, 0, 1), 500.0), stepped_vertex(-11, 3, (9, 9, 9), (1, 0, 0), 5.0), \
        stepped_vertex(22, 2, (0, 0, 0), (0, 1, 0), 1.0)
    bare = event.Vertex('mu-', (0, 0, 0), (0, 0, 1), 1.0, pdgcode=13)
    seg = steps.segments_from_vertices([mu, bare, e, gamma], evidx=[4, 5, 6, 7])
    assert len(seg) == 6 + 3 + 2 and np.array_equal(seg.evidx, [4] * 6 + [6] * 3 + [7] * 2)
    # no segment joins two vertices: every one is 5 mm long
    assert np.allclose(np.linalg.norm(seg.b - seg.a, axis=1), 5.0)
    assert np.array_equal(seg.z, [-1] * 6 + [1] * 3 + [0] * 2) and (seg.beta[9:] == 0).all()
    gam = 1 + np.array([500.0, 499.0]) / 105.6583755
    assert np.isclose(seg.beta[0], np.sqrt(1 - 1 / gam ** 2).mean(), rtol=1e-6)
    assert np.allclose(seg.qedep, 0.8) and np.isclose(seg.t_b[0] - seg.t_a[0], 5.0 / 299.79, rtol=1e-4)


def test_batching_does_not_change_the_photons():
    src = steps.LightSource(medium(SLOPED_N, spectrum=True, light_yield=30.0, waveform=True), WL)
    vertices = [stepped_vertex(13, 40, (0, 0, 0), (0, 0.6, 0.8), 300.0), stepped_vertex(11, 25, (50, 0, -20), (1, 0, 0), 30.0, t0=3.0)]
    whole = steps.segments_from_vertices(vertices, evidx=[0, 1], segment_base=500)
    one = steps.generate_photons(whole, src, SEED)
    assert set(np.unique(one.flags)) == {event.CHERENKOV, event.SCINTILLATION} and set(np.unique(one.evidx)) == {0, 1}
    three = event.Photons.join([steps.generate_photons(whole[lo:hi], src, SEED) for lo, hi in ((0, 7), (7, 41), (41, 65))])
    assert whole[7:41].segment_base == 507 and len(one) == len(three) > 1000
    for name in ('pos', 'dir', 'pol', 'wavelengths', 't', 'flags', 'last_hit_triangles', 'weights', 'evidx'):
        assert np.array_equal(getattr(one, name).view(np.uint32), getattr(three, name).view(np.uint32)), name
    # ... and it does change them with the base and with the seed
    assert not np.array_equal(steps.generate_photons(whole[0:7], src, SEED + 1).pos[:5], one.pos[:5])
    # Cherenkov photons come before scintillation photons in every segment
    offsets, _ = steps.count_photons(whole, src, SEED)
    for k in (0, 20, 64):
        f = one.flags[offsets[2 * k]:offsets[2 * k + 2]]
        assert (f[:offsets[2 * k + 1] - offsets[2 * k]] == event.CHERENKOV).all() and (f[offsets[2 * k + 1] - offsets[2 * k]:] == event.SCINTILLATION).all()


def test_capacity_and_bad_sources_are_refused():
    import ctypes
    from chroma_amd import _lib
    src = steps.LightSource(medium(1.5, spectrum=True, light_yield=50.0), WL)
    seg = identical(20, 1.0, qedep=0.2)
    offsets, total = steps.count_photons(seg, src, SEED)
    n = int(total)
    guard = 8
    arrays, host = _lib.PhotonArrays(), {}
    for name, width, dtype in (('pos', 3, f32), ('dir', 3, f32), ('pol', 3, f32), ('wavelengths', 1, f32), ('t', 1, f32), ('flags', 1, np.uint32),
                               ('last_hit_triangles', 1, np.int32), ('weights', 1, f32), ('evidx', 1, np.uint32), ('rng_counters', 1, np.uint32)):
        host[name] = np.full((n + guard) * width, 7, dtype=dtype)
        setattr(arrays, name, _lib.ptr(host[name]))
    s = seg.struct()
    lib = _lib.load()
    assert lib.chroma_steps_generate_host(ctypes.byref(src.struct), ctypes.byref(s), SEED, _lib.ptr(offsets), ctypes.byref(arrays), n - 1) == -1
    assert all((a == 7).all() for a in host.values())
    assert lib.chroma_steps_generate_host(ctypes.byref(src.struct), ctypes.byref(s), SEED, _lib.ptr(offsets), ctypes.byref(arrays), n) == 0
    assert all((a[len(a) // (n + guard) * n:] == 7).all() for a in host.values()) and (host['weights'][:n] == 1).all()
    with pytest.raises(ValueError):
        steps.LightSource(medium(1.5), WL, cherenkov_range=(300, 301))
    with pytest.raises(ValueError):
        steps.LightSource(Material('nothing'), WL)
