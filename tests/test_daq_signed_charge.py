"""The DAQ on a detector whose charge CDF starts below zero, without a GPU: the C oracle's run_daq and run_daq_many and the
library's chroma_daq_noise_host are the Python restatements bit for bit -- time bits, charge counts, histories.

The charge count is cm_f2u32(cm_roundf(charge / charge_unit)): NaN and negatives give 0, saturating, as the device's
v_cvt_u32_f32.  The restatements clamp in Python integers (``charge_count`` of tests/test_daq_pulses_host.py).  A raw C cast of
the rounded quotient is undefined for a negative charge; a host compiler wraps it, the wrapped count subtracts from the
channel's sum, and this module fails: on the commit before the clamp every case with a negative draw failed on its charge counts
(12 of the 14 oracle and twin cases; the other two are single photons that drew a positive charge).

The detectors, photons and input conditions are tests/signed_charge.py's; tests/test_gpu_daq_signed_charge.py runs the same
cases on the device.
"""
import numpy as np
import pytest

from test_gpu_photon_arrays import daq_tables, DAQ_BASE
from test_gpu_daq_events import oracle_rows, BASE, WEIGHT
from test_daq_pulses_host import restate, SEED, F
from signed_charge import (signed_geos, signed_rows, event_bounds, whole, restate_many, reduce_words, assert_shares, max_count,          # noqa: F401
                           restate_signed_noise, noise_tables, KINDS, SIZES, NDAQ, WINDOW)


@pytest.fixture(scope='module')
def signed_cases(oracle_mod, signed_geos):
    """The restated accepted photons, once per case and shared read-only: signed_cases(kind, n, route) -> (rows, bounds, acc) with
    route 'one' (one acquisition of every photon), 'many' (NDAQ copies) or 'events' (three rows)."""
    cache = {}

    def get(kind, n, route):
        if (kind, n, route) not in cache:
            geo = signed_geos[kind]
            rows = signed_rows(geo, n)
            if route == 'many':
                bounds, acc = None, restate_many(oracle_mod, geo, rows[0])
            else:
                bounds = whole(n) if route == 'one' else event_bounds(n)
                acc = restate(oracle_mod, geo, rows[0], bounds, signed=True)
            cache[kind, n, route] = (rows, bounds, acc)
        return cache[kind, n, route]
    return get


@pytest.mark.parametrize('route', ['one', 'many', 'events'])
@pytest.mark.parametrize('kind', KINDS)
def test_the_inputs_draw_negative_and_positive_charges_and_the_first_edge(signed_geos, signed_cases, kind, route):
    rows, bounds, acc = signed_cases(kind, 4097, route)
    assert_shares(acc, kind, '%s, %s' % (kind, route), least=400)
    assert max_count(signed_geos[kind]) == 65536
    one = signed_cases(kind, 1, route)[2]
    assert len(one) == (NDAQ if route == 'many' else 1), 'the one photon is accepted under every stream'


def assert_words(got, want, what):
    for a, b, name in zip(got, want, ('time bits', 'charge counts', 'histories')):
        assert np.array_equal(a, b), '%s: %s' % (what, name)


def assert_sums_hold(q, npe, top, what):
    """what wrapping breaks: a word's count is at most ``top`` per photoelectron"""
    assert (q.astype(np.uint64) <= np.uint64(top) * npe).all(), '%s: a word holds more than %d per photoelectron' % (what, top)


@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('kind', KINDS)
def test_the_oracles_run_daq_is_the_restatement(oracle_mod, signed_geos, signed_cases, kind, n):
    geo = signed_geos[kind]
    rows, bounds, acc = signed_cases(kind, n, 'one')
    tables, unit = daq_tables(geo)
    state = oracle_mod.daq_state(geo.nchannels)
    oracle_mod.run_daq(geo.packed, rows[0], tables, unit, seed=SEED, photon_id_base=DAQ_BASE, acquisition=BASE, weight=WEIGHT, state=state)
    want = reduce_words(acc, 1, geo.nchannels)
    what = '%s, %d photons' % (kind, n)
    assert_words(state, want, what)
    assert_sums_hold(state[1], want[3], max_count(geo), what)


@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('kind', KINDS)
def test_the_oracles_run_daq_many_is_the_restatement(oracle_mod, signed_geos, signed_cases, kind, n):
    geo = signed_geos[kind]
    rows, bounds, acc = signed_cases(kind, n, 'many')
    tables, unit = daq_tables(geo)
    state = oracle_mod.daq_state(NDAQ * geo.nchannels)
    oracle_mod.run_daq_many(geo.packed, rows[0], tables, unit, seed=SEED, ndaq=NDAQ, photon_id_base=DAQ_BASE, acquisition=BASE, weight=WEIGHT, state=state)
    want = reduce_words(acc, NDAQ, geo.nchannels)
    what = '%s, %d photons, %d copies' % (kind, n, NDAQ)
    assert_words(state, want, what)
    assert_sums_hold(state[1], want[3], max_count(geo), what)


@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('kind', KINDS)
def test_the_oracles_run_daq_row_by_row_is_the_restatement(oracle_mod, signed_geos, signed_cases, kind, n):
    geo = signed_geos[kind]
    rows, bounds, acc = signed_cases(kind, n, 'events')
    state = oracle_rows(oracle_mod, geo, rows[0], bounds)
    want = reduce_words(acc, len(bounds) - 1, geo.nchannels)
    what = '%s, %d photons, three rows' % (kind, n)
    assert_words(state, want, what)
    assert_sums_hold(state[1], want[3], max_count(geo), what)


@pytest.mark.parametrize('kind', KINDS)
def test_the_noise_host_twin_is_the_restatement(oracle_mod, signed_geos, kind):
    geo = signed_geos[kind]
    (tx, ty, qx, qy), unit = daq_tables(geo)
    noise, count_cdf, accept = noise_tables(geo)
    nrows = 3
    want, charge = restate_signed_noise(oracle_mod, geo, count_cdf, accept, WINDOW, nrows)
    drawn = np.zeros(len(want), dtype=[('charge', F), ('charge_int', np.uint32)])
    drawn['charge'], drawn['charge_int'] = charge, want['charge_int']
    assert_shares(drawn, kind, '%s, noise' % kind, least=60)
    got = noise.sample(WINDOW, nrows, geo.nchannels, (qx, qy), unit, seed=SEED, acquisition=BASE)
    assert len(got) == len(want)
    for name in ('row', 'channel', 'bin', 'charge_int'):
        assert np.array_equal(got[name].astype(np.int64), want[name].astype(np.int64)), '%s: %s' % (kind, name)
    assert np.array_equal(got['time'].view(np.uint32), want['time'].view(np.uint32)), kind + ': time bits'
    assert got['charge_int'].max() <= max_count(geo)
