"""Detectors whose charge CDF starts below zero, their photons, and the restatements the DAQ is held to on them (no test here: a
helper of tests/test_daq_signed_charge.py, tests/test_gpu_daq_signed_charge.py and tests/test_host_twins_sanitized.py).

A pedestal-subtracted single-photoelectron spectrum has a negative tail, and ``Detector.set_charge_dist_gaussian`` takes any
lower edge.  The charge count of such a draw is cm_f2u32(cm_roundf(charge / charge_unit)): 0 for every negative charge.  A raw C
cast there is undefined: a host compiler wraps (a count of some 2^32 - 16384 that SUBTRACTS from the channel's sum), the device
saturates.  The detectors are ``demo.tiny()``'s channels under two charge tables:

  'table'     hand-made: edges from -1.0 to 2.0, the first bin with 12 % of the mass.  ``Detector._pdf_to_cdf`` starts cdf_y at
              the first bin's content, not at 0 (the reference's quirk), so a draw at or below cdf_y[0] returns edges[0] = -1.0
              exactly and bin k + 1's mass is spread over bin k's edges.
  'gaussian'  ``set_charge_dist_gaussian(0.3, 0.6, -1.0, 2.0)``.

The photons are written in NumPy (no propagation): n = 1 (weight 2: accepted under every stream) and n = 4097 (weights in
[0, 1]), both under the global weight 0.7 of the DAQ tests.  ``assert_shares`` states what the inputs must do; the tests call it.
"""
import copy

import numpy as np
import pytest

from test_gpu_photon_arrays import _Geo, make_photons, draw_triangles, draw_flags, daq_tables, DETECT, DAQ_BASE
from test_gpu_daq_events import BASE, WEIGHT, RESET_BITS
from test_daq_pulses_host import uniform, interp_table, roundf, charge_count, restate, SEED, F

KINDS = ('table', 'gaussian')
SIZES = (1, 4097)                    # DAQ_PULSES_SPAN is 1024 and a block 256: one lane; four spans and a photon
NDAQ = 3
EDGES = np.array([-1.0, -0.75, -0.5, -0.25, 0.0, 0.5, 1.0, 1.5, 2.0])
CONTENTS = np.array([0.12, 0.10, 0.10, 0.10, 0.18, 0.20, 0.15, 0.05])
WINDOW = (-16.0, 0.25, 128)          # holds every accepted time


def signed_geometry(tiny_geometry, kind):
    """``tiny_geometry`` (shared, left as it is) under a signed charge table: a shallow copy with its own charge_cdf."""
    from chroma_amd.detector import Detector
    det = copy.copy(tiny_geometry)
    if kind == 'table':
        det.charge_cdf = Detector._pdf_to_cdf(EDGES, CONTENTS)
    else:
        det.set_charge_dist_gaussian(0.3, 0.6, -1.0, 2.0)
    assert det.charge_cdf[0][0] == -1.0 and det.charge_cdf[0][-1] == 2.0 and tiny_geometry.charge_cdf[0][0] >= 0.0
    return det


@pytest.fixture(scope='module')
def signed_geos(tiny_geometry, tiny_packed):
    """{kind: the detector with what NumPy needs} (the packed geometry holds no charge table: it is tiny's)."""
    return {kind: _Geo(signed_geometry(tiny_geometry, kind), tiny_packed) for kind in KINDS}


def max_count(geo):
    """The largest count one photoelectron can add: that of the table's last edge (65536)."""
    (tx, ty, qx, qy), unit = daq_tables(geo)
    return charge_count(roundf(F(qx[-1] / F(unit))))


def signed_rows(geo, n, seed=81):
    """(event.Photons, draw counters) of n photons: triangles on channels, on none and none at all, histories with and without
    the detection bit, times around 0 (some smeared times are negative too).  n = 1: a detected photon on a channel, weight 2."""
    rng = np.random.default_rng(seed)
    rows = make_photons(rng, n)
    ph = rows[0]
    ph.flags[:] = draw_flags(rng, n, DETECT, p=0.85)
    ph.last_hit_triangles[:] = draw_triangles(rng, geo, n)
    ph.t[:] = rng.uniform(-3.0, 3.0, n).astype(np.float32)
    if n == 1:
        ph.flags[:] |= np.uint32(DETECT)
        ph.last_hit_triangles[:] = geo.on[len(geo.on) // 2]
        ph.weights[:] = 2.0
    return rows


def event_bounds(n):
    """Three rows, one of them (n = 1: two) empty."""
    return np.array([0, 0, 1, 1] if n == 1 else [0, 1500, 1500, n], dtype=np.uint32)


def whole(n):
    return np.array([0, n], dtype=np.uint32)


def restate_many(oracle_mod, geo, ph, ndaq=NDAQ, acquisition=BASE, weight=WEIGHT, seed=SEED, id_base=DAQ_BASE):
    """run_daq_many restated as ``restate`` restates run_daq: copy c of a photon draws from words 8 c ... of the photon's stream
    -- the gate, the two words of the jitter, the time smear, the charge; 'row' is the copy.  The normal deviate itself is the
    oracle's (``rng_probe``): what is restated is the draw order, the tables and the count."""
    (tx, ty, qx, qy), unit = daq_tables(geo)
    unit, weight = F(unit), F(weight)
    key = (seed & 0xffffffff, seed >> 32)
    stream = (1 + acquisition) & 0xffffffff
    out = []
    for i in range(len(ph)):
        triangle = int(ph.last_hit_triangles[i])
        if triangle <= -1:
            continue
        channel = int(geo.channel_of_triangle[triangle])
        history = int(ph.flags[i])
        if channel < 0 or not history & DETECT:
            continue
        pid = id_base + i
        for c in range(ndaq):
            first = oracle_mod.philox((2 * c, stream, pid & 0xffffffff, pid >> 32), key)           # words 8 c .. 8 c + 3
            if not uniform(first[0]) < F(ph.weights[i] * weight):
                continue
            second = oracle_mod.philox((2 * c + 1, stream, pid & 0xffffffff, pid >> 32), key)      # words 8 c + 4 ..
            jitter = oracle_mod.rng_probe('rng_normal', [key[0], key[1], pid & 0xffffffff, pid >> 32, stream, 8 * c + 1])[0, 0]
            time = F(F(ph.t[i] + jitter) + interp_table(uniform(first[3]), ty, tx))
            charge = interp_table(uniform(second[0]), qy, qx)
            out.append((i, c, channel, time, charge_count(roundf(F(charge / unit))), history, charge))
    dtype = [('photon', np.int64), ('row', np.int64), ('channel', np.int64), ('time', F), ('charge_int', np.uint32), ('history', np.uint32),
             ('charge', F)]
    acc = np.array(out, dtype=dtype)
    acc.flags.writeable = False
    return acc


def reduce_words(acc, nrows, stride):
    """(time bits, charge counts, histories, photoelectrons) per word row * stride + channel, reduced the way run_daq reduces:
    the unsigned minimum of the time bits against the reset value, the sum of the CLAMPED counts (wrapping), the OR."""
    word = acc['row'] * stride + acc['channel']
    t = np.full(nrows * stride, RESET_BITS, dtype=np.uint32)
    np.minimum.at(t, word, acc['time'].view(np.uint32))
    q = np.zeros(nrows * stride, dtype=np.uint64)
    np.add.at(q, word, acc['charge_int'].astype(np.uint64))
    hist = np.zeros(nrows * stride, dtype=np.uint32)
    np.bitwise_or.at(hist, word, acc['history'])
    npe = np.bincount(word, minlength=nrows * stride).astype(np.uint64)
    assert (q < 2 ** 32).all(), 'the sums of these cases do not wrap: a word that did would hide a wrapped count'
    return t, q.astype(np.uint32), hist, npe


def assert_shares(acc, kind, what, least=100):
    """What the inputs are there for: of the accepted photons (or kept noise) at least 20 % draw a negative charge and at least
    20 % a positive one; on the hand-made table at least 5 % return edges[0] exactly.  Every negative draw counts 0."""
    n = len(acc)
    assert n >= least, '%s: %d accepted' % (what, n)
    negative, positive = (acc['charge'] < 0).sum(), (acc['charge'] > 0).sum()
    assert negative >= 0.2 * n and positive >= 0.2 * n, '%s: %d negative and %d positive of %d' % (what, negative, positive, n)
    if kind == 'table':
        assert (acc['charge'] == F(EDGES[0])).sum() >= 0.05 * n, '%s: %d of %d at the first edge' % (what, (acc['charge'] == F(EDGES[0])).sum(), n)
    assert (acc['charge_int'][acc['charge'] < 0] == 0).all() and (acc['charge_int'][acc['charge'] > F(0.01)] > 0).all(), what


def restate_signed_noise(oracle_mod, geo, count_cdf, accept, window, nrows, base=BASE, seed=SEED):
    """``restate_noise`` of tests/test_daq_noise_host.py on the detector's signed table, with the drawn charge beside the count
    (the charge is drawn again from the candidate's word c, as that function draws it)."""
    from test_daq_noise_host import restate_noise
    tables = daq_tables(geo)
    kept, drawn, thinned = restate_noise(oracle_mod, count_cdf, accept, tables, window, nrows, geo.nchannels, base=base, seed=seed)
    (tx, ty, qx, qy), unit = tables
    key = (seed & 0xffffffff, seed >> 32)
    charge = np.zeros(len(kept), dtype=F)
    for k, pe in enumerate(kept):
        w = 3 + 3 * int(pe['candidate'])
        words = oracle_mod.philox((w >> 2, (1 + base + int(pe['row'])) & 0xffffffff, int(pe['channel']), 0xffffffff), key)
        charge[k] = interp_table(uniform(words[w & 3]), qy, qx)
    return kept, charge


def noise_tables(geo, window=WINDOW, mu=2.5):
    """(DaqNoise, count_cdf, accept) of the noise tests' rate pattern at ``mu`` candidates per word."""
    from test_daq_noise_host import PATTERN
    from chroma_amd.gpu.daq import DaqNoise
    top = mu / (1e-9 * window[2] * float(F(window[1])))
    noise = DaqNoise(top * np.resize(np.array(PATTERN), geo.nchannels))
    count_cdf, accept = noise.tables(window, geo.nchannels)
    return noise, count_cdf, accept
