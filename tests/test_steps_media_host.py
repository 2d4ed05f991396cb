"""Photons from charged-particle steps with a medium per segment, host twin (chroma_steps_count_media_host /
chroma_steps_generate_media_host): segment s in medium m emits, bit for bit, what the single-medium host call emits for
segment s from medium m's LightSource.  No GPU."""
import ctypes

import numpy as np
import pytest

from chroma_amd import _lib, event
from chroma_amd.generator import steps
from chroma_amd.geometry import Material, standard_wavelengths

SEED = 0x0F1E2D3C4B5A6978
WL = standard_wavelengths.astype(np.float64)
FIELDS = ('pos', 'dir', 'pol', 'wavelengths', 't', 'flags', 'last_hit_triangles', 'weights', 'evidx')
BASE = 987654321098


def material(name, n0, light_yield=None, waveform=True, peak=430.0):
    m = Material(name)
    m.set('refractive_index', n0 - (WL - 200.0) * 5e-5)
    m.set('absorption_length', 1e6)
    m.set('scattering_length', 1e6)
    if light_yield:
        m.set('scintillation_spectrum', np.where(np.abs(WL - peak) < 50, 1.0 + np.cos((WL - peak) * np.pi / 50), 0.0))
        m.scintillation_light_yield = light_yield
        if waveform:
            t = np.arange(0, 1000, 0.05)
            m.scintillation_waveform = np.column_stack([t, 0.7 * np.exp(-t / 3.0) / 3.0 + 0.3 * np.exp(-t / 12.0) / 12.0])
    return m


def three_media():
    """Cherenkov light only; scintillating with a waveform; scintillating promptly"""
    return steps.LightMedia([material('water', 1.36), material('scintillator', 1.52, 120.0), material('glass', 1.47, 40.0, waveform=False, peak=390.0)], WL)


def mixed_segments(n, seed=7, segment_base=BASE):
    """A broken track of n segments: beta either side of every medium's threshold, charges 0, +-1 and 2, no deposit, a small one,
    and one whose mean count is far beyond 16 (the switch of the count from Knuth's product to the rounded normal)."""
    rng = np.random.default_rng(seed)
    x = np.cumsum(rng.normal(0, 1.5, (n + 1, 3)), axis=0)
    t = np.cumsum(rng.uniform(0.001, 0.02, n + 1))
    beta = rng.choice([0.3, 0.66, 0.7, 0.8, 0.95, 0.9999], n)
    z = rng.choice([0.0, 1.0, -1.0, 2.0], n)
    qedep = rng.choice([0.0, 0.02, 0.1, 1.5], n)
    return steps.Segments(x[:-1], x[1:], t[:-1], t[1:], beta, z, qedep, rng.integers(0, 5, n), segment_base=segment_base)


def mixed_medium(n, nmedia=3, seed=11):
    """rows -1 .. nmedia: both ends are outside the table"""
    return np.random.default_rng(seed).integers(-1, nmedia + 1, n).astype(np.int32)


def assert_same_photons(a, b):
    assert len(a) == len(b)
    for name in FIELDS:
        assert np.array_equal(getattr(a, name).view(np.uint32), getattr(b, name).view(np.uint32)), name


@pytest.fixture(scope='module')
def media():
    return three_media()


@pytest.fixture(scope='module')
def case(media):
    seg, medium = mixed_segments(257), mixed_medium(257)
    assert set(np.unique(medium)) == {-1, 0, 1, 2, 3}
    offsets, total = steps.count_photons(seg, media, SEED, medium=medium)
    return seg, medium, offsets, total, steps.generate_photons(seg, media, SEED, medium=medium)


def test_each_segment_emits_what_its_mediums_source_emits(media, case):
    seg, medium, offsets, total, got = case
    assert offsets[0] == 0 and offsets[-1] == total == len(got) and total >= 3 * 256
    counts = np.diff(offsets.astype(np.int64))
    assert (counts >= 0).all()
    checked = set()
    for m, source in enumerate(media.sources):
        want_offsets, _ = steps.count_photons(seg, source, SEED)
        want = steps.generate_photons(seg, source, SEED)
        for s in np.flatnonzero(medium == m):
            lo, mid, hi = (int(x) for x in offsets[2 * s:2 * s + 3])
            wlo, wmid, whi = (int(x) for x in want_offsets[2 * s:2 * s + 3])
            assert (mid - lo, hi - mid) == (wmid - wlo, whi - wmid), (m, s)
            assert_same_photons(got[lo:hi], want[wlo:whi])
            if hi - lo:
                checked.add((m, bool(mid - lo), bool(hi - mid), (hi - lo) > 40))
    # every medium was seen with photons; the scintillating ones with both kinds, and with counts from the normal branch
    assert {m for m, _, _, _ in checked} == {0, 1, 2}
    assert (1, True, True, True) in checked and any(c[0] == 2 and c[2] for c in checked) and not any(c[0] == 0 and c[2] for c in checked)
    for s in np.flatnonzero((medium < 0) | (medium >= len(media))):
        assert counts[2 * s] == 0 and counts[2 * s + 1] == 0
    assert {event.CHERENKOV, event.SCINTILLATION} == set(np.unique(got.flags))
    # the prompt medium adds no delay: its scintillation photons lie within their segment's time span
    for s in np.flatnonzero(medium == 2):
        t = got.t[int(offsets[2 * s + 1]):int(offsets[2 * s + 2])]
        assert ((t >= seg.t_a[s]) & (t <= seg.t_b[s])).all()


def test_two_calls_with_consecutive_bases_give_the_same_photons(media, case):
    seg, medium, offsets, total, whole = case
    cut = 100
    parts = [steps.generate_photons(seg[:cut], media, SEED, medium=medium[:cut]), steps.generate_photons(seg[cut:], media, SEED, medium=medium[cut:])]
    assert seg[cut:].segment_base == BASE + cut and len(parts[0]) == offsets[2 * cut]
    assert_same_photons(event.Photons.join(parts), whole)


def test_no_segments(media):
    offsets, total = steps.count_photons(steps.Segments.join([]), media, SEED, medium=np.zeros(0, np.int32))
    assert np.array_equal(offsets, [0]) and total == 0
    assert len(steps.generate_photons(steps.Segments.join([]), media, SEED, medium=[])) == 0


def test_a_bad_table_is_refused_with_a_message(case):
    seg, medium = case[0], case[1]

    def refused(media, match):
        offsets = np.zeros(2 * len(seg) + 1, np.uint32)
        total = ctypes.c_uint64()
        s = seg.struct()
        lib = _lib.load()
        rc = lib.chroma_steps_count_media_host(ctypes.byref(media.desc), ctypes.byref(s), _lib.ptr(medium), SEED, _lib.ptr(offsets), ctypes.byref(total))
        assert rc == -1 and match in lib.chroma_last_error(), lib.chroma_last_error()
        arrays = _lib.PhotonArrays()
        rc = lib.chroma_steps_generate_media_host(ctypes.byref(media.desc), ctypes.byref(s), _lib.ptr(medium), SEED, _lib.ptr(offsets), ctypes.byref(arrays), 0)
        assert rc == -1 and match in lib.chroma_last_error()
        with pytest.raises(_lib.ChromaError, match=match.decode()):
            steps.count_photons(seg, media, SEED, medium=medium)

    bad = three_media()
    j = int(np.searchsorted(bad.scintillation_cdf[1], 0.5))
    bad.scintillation_cdf[1, j] = bad.scintillation_cdf[1, j - 1] - 1e-3          # a step down inside a row that is read
    refused(bad, b'scintillation CDF row')
    bad = three_media()
    bad.time_cdf[1, 5000] = 0.0
    refused(bad, b'time CDF row')
    bad = three_media()
    bad.desc.cherenkov_lo = bad.desc.cherenkov_hi
    refused(bad, b'Cherenkov range')
    bad.desc.cherenkov_lo = bad.desc.cherenkov_hi + 1
    refused(bad, b'Cherenkov range')
    # rows that are not read may hold anything: the CDF rows of the medium without a yield, the time row of the prompt one
    fine = three_media()
    fine.scintillation_cdf[0, :] = np.nan
    fine.time_cdf[0, :] = -1.0
    fine.time_cdf[2, ::2] = 7.0
    assert_same_photons(steps.generate_photons(seg, fine, SEED, medium=medium), case[4])


def test_medium_goes_with_media_only(media, case):
    seg, medium = case[0], case[1]
    with pytest.raises(ValueError, match='medium='):
        steps.count_photons(seg, media, SEED)
    with pytest.raises(ValueError, match='medium='):
        steps.count_photons(seg, media.sources[0], SEED, medium=medium)
    want = sum(media.sources[m].expected_photons(seg[s:s + 1]) for s, m in enumerate(medium) if 0 <= m < 3)
    assert media.expected_photons(seg, medium) == pytest.approx(want, rel=1e-12)
    assert media.expected_at_most(seg) >= max(want, max(s.expected_photons(seg) for s in media.sources))


def test_media_of_a_geometry_have_a_row_per_material_in_its_order():
    from conftest import make_stress_geometry
    geometry = make_stress_geometry()
    media = steps.LightMedia.from_geometry(geometry)
    assert len(media) == len(geometry.unique_materials) == media.desc.nmedia > 1
    for m, (mat, source) in enumerate(zip(geometry.unique_materials, media.sources)):
        assert source.material is mat and media.index(mat) == m
        assert np.array_equal(media.refractive_index[m], source.refractive_index)
        assert media.light_yield[m] == np.float32(source.light_yield) and bool(media.prompt[m]) == (source.time_cdf is None)
