"""The DAQ's charge draw on the GPU on a detector whose charge CDF starts below zero: all five routes of the draw, bit for bit on
the C oracle, on the Python restatements and on the host twin that tests/test_daq_signed_charge.py holds to one another.

  chroma_daq_acquire                                    k_run_daq
  chroma_daq_acquire_many, ndaq = 3                     k_run_daq_many
  chroma_daq_acquire_events + chroma_daq_compact_events k_run_daq_events
  chroma_daq_count_pulses / chroma_daq_acquire_pulses   daq_pulse_photon (kernels_daq_pulses.h)
  chroma_daq_acquire_pulses_noise                       daq_noise::photoelectron (daq_noise_common.h), against chroma_daq_noise_host

A negative charge counts 0 (cm_f2u32); the device's v_cvt_u32_f32 did that before the kernels said so, a host compiler's cast
wraps.  Beside the bits, the property that a wrapped count breaks: every word's q_int is the sum of its clamped counts and at
most 65536 per photoelectron.  The photons are written in NumPy: n = 1 and n = 4097 (DAQ_PULSES_SPAN is 1024, a block 256), the
per-event calls on three rows with an empty one.  No propagation runs.
"""
import ctypes

import numpy as np
import pytest

from test_gpu_photon_arrays import gpu, upload, daq_tables, call, structure, DAQ_BASE, DETECT, SENTINEL, GUARD_WORDS          # noqa: F401
from test_gpu_daq_events import (tables_of, device_state, acquire_events, assert_state, compact, expected_sparse, assert_sparse, oracle_rows,
                                 BASE, WEIGHT)
from test_gpu_daq_pulses import Outputs, assert_pulses, acquire_rc, count_rc
from test_gpu_daq_noise import Noise, row_noise_words, count_noise_rc, acquire_noise_rc, assert_row_noise
from test_daq_pulses_host import expected_pulses, SEED
from test_daq_noise_host import expected_with_noise
from test_daq_signed_charge import signed_cases, assert_words, assert_sums_hold          # noqa: F401
from signed_charge import (signed_geos, assert_shares, reduce_words, max_count, noise_tables, KINDS, SIZES, NDAQ, WINDOW)          # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def geos(gpu, signed_geos):
    """The signed detectors on the device (tiny's packed geometry under their own charge tables)."""
    for geo in signed_geos.values():
        if geo.gg is None:
            geo.gg = gpu.GPUDetector(geo.geometry, packed=geo.packed)
            assert geo.gg.nchannels == geo.nchannels
    return signed_geos


def check_inputs(acc, kind, n, what):
    if n > 1:
        assert_shares(acc, kind, what, least=400)
    else:
        assert len(acc) >= 1, what + ': the one photon is not accepted'


@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('kind', KINDS)
def test_acquire_is_the_oracle_and_the_restatement(gpu, oracle_mod, geos, signed_cases, kind, n):
    from chroma_amd import _lib
    geo = geos[kind]
    rows, bounds, acc = signed_cases(kind, n, 'one')
    what = '%s, %d photons' % (kind, n)
    check_inputs(acc, kind, n, what)
    daq = tables_of(gpu, geo)
    words = geo.nchannels
    arrays = device_state(gpu, words)
    call(gpu, 'chroma_daq_reset', 1e9, words, arrays[0].ptr, arrays[1].ptr, arrays[2].ptr)
    dev = upload(rows)
    s = structure(dev)
    call(gpu, 'chroma_daq_acquire', geo.gg.handle, ctypes.byref(daq.tables), 0, n, DETECT, ctypes.byref(s), _lib.Rng(SEED, DAQ_BASE), BASE, WEIGHT,
         arrays[0].ptr, arrays[1].ptr, arrays[2].ptr)
    state = oracle_mod.daq_state(words)
    oracle_mod.run_daq(geo.packed, rows[0], daq._tables_host, daq.charge_unit, seed=SEED, photon_id_base=DAQ_BASE, acquisition=BASE, weight=WEIGHT, state=state)
    want = reduce_words(acc, 1, words)
    assert_words(state, want, what + ': the oracle is not the restatement')
    assert_state(arrays, want[:3], words, what)
    assert_sums_hold(arrays[1].get()[:words], want[3], max_count(geo), what)


@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('kind', KINDS)
def test_acquire_many_is_the_oracle_and_the_restatement(gpu, oracle_mod, geos, signed_cases, kind, n):
    from chroma_amd import _lib
    geo = geos[kind]
    rows, bounds, acc = signed_cases(kind, n, 'many')
    what = '%s, %d photons, %d copies' % (kind, n, NDAQ)
    check_inputs(acc, kind, n, what)
    daq = tables_of(gpu, geo)
    words = NDAQ * geo.nchannels
    arrays = device_state(gpu, words)
    call(gpu, 'chroma_daq_reset', 1e9, words, arrays[0].ptr, arrays[1].ptr, arrays[2].ptr)
    dev = upload(rows)
    s = structure(dev)
    call(gpu, 'chroma_daq_acquire_many', geo.gg.handle, ctypes.byref(daq.tables), 0, n, DETECT, ctypes.byref(s), _lib.Rng(SEED, DAQ_BASE), BASE, WEIGHT,
         NDAQ, geo.nchannels, arrays[0].ptr, arrays[1].ptr, arrays[2].ptr)
    state = oracle_mod.daq_state(words)
    oracle_mod.run_daq_many(geo.packed, rows[0], daq._tables_host, daq.charge_unit, seed=SEED, ndaq=NDAQ, photon_id_base=DAQ_BASE, acquisition=BASE,
                            weight=WEIGHT, state=state)
    want = reduce_words(acc, NDAQ, geo.nchannels)
    assert_words(state, want, what + ': the oracle is not the restatement')
    assert_state(arrays, want[:3], words, what)
    assert_sums_hold(arrays[1].get()[:words], want[3], max_count(geo), what)


@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('kind', KINDS)
def test_acquire_events_and_the_compaction_are_the_oracle_and_the_restatement(gpu, oracle_mod, geos, signed_cases, kind, n):
    geo = geos[kind]
    rows, bounds, acc = signed_cases(kind, n, 'events')
    what = '%s, %d photons, three rows' % (kind, n)
    check_inputs(acc, kind, n, what)
    nrows, nch = len(bounds) - 1, geo.nchannels
    words = nrows * nch
    daq = tables_of(gpu, geo)
    arrays = device_state(gpu, words)
    call(gpu, 'chroma_daq_reset', 1e9, words, arrays[0].ptr, arrays[1].ptr, arrays[2].ptr)
    acquire_events(gpu, geo, daq, upload(rows), bounds, arrays)
    state = oracle_rows(oracle_mod, geo, rows[0], bounds)
    want = reduce_words(acc, nrows, nch)
    assert_words(state, want, what + ': the oracle is not the restatement')
    assert_state(arrays, want[:3], words, what)
    assert_sums_hold(arrays[1].get()[:words], want[3], max_count(geo), what)
    sparse = expected_sparse(geo, want[:3], nrows)
    capacity = len(sparse[1]) + 3
    ntouched, got = compact(gpu, geo, arrays, nrows, capacity, daq.charge_unit)
    assert_sparse(got, ntouched, sparse, nrows, capacity, what)
    empty = np.flatnonzero(np.diff(bounds.astype(np.int64)) == 0)
    assert len(empty) >= 1 and (np.diff(sparse[0].astype(np.int64))[empty] == 0).all()


@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('kind', KINDS)
def test_count_and_acquire_pulses_are_the_restatement(gpu, geos, signed_cases, kind, n):
    from chroma_amd import _lib
    geo = geos[kind]
    rows, bounds, acc = signed_cases(kind, n, 'events')
    what = '%s, %d photons, three rows' % (kind, n)
    check_inputs(acc, kind, n, what)
    nrows = len(bounds) - 1
    want = expected_pulses(acc, WINDOW, nrows, geo.nchannels)
    assert want['naccepted'] == len(acc), what + ': the window does not hold every accepted photon'
    daq = tables_of(gpu, geo)
    dev = upload(rows)
    rc, naccepted = count_rc(gpu, geo, daq, dev, bounds, WINDOW)
    _lib.check(rc)
    assert naccepted == want['naccepted'], what
    out = Outputs(nrows, naccepted)
    rc, npulses = acquire_rc(gpu, out, geo, daq, dev, bounds, WINDOW)
    _lib.check(rc)
    assert_pulses(out, npulses, want, what)
    got = out.get()
    assert_sums_hold(got['q_int'][:npulses], got['npe'][:npulses].astype(np.uint64), max_count(geo), what)
    # the pulses of a word sum to the word of the channel routes
    row = np.repeat(np.arange(nrows), np.diff(want['offsets'].astype(np.int64)))
    q = np.zeros(nrows * geo.nchannels, dtype=np.uint64)
    np.add.at(q, row * geo.nchannels + got['channel'][:npulses].view(np.int32), got['q_int'][:npulses].astype(np.uint64))
    assert np.array_equal(q.astype(np.uint32), reduce_words(acc, nrows, geo.nchannels)[1]), what


@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('kind', KINDS)
def test_acquire_pulses_noise_is_the_photons_and_the_host_twins_noise(gpu, geos, signed_cases, kind, n):
    from chroma_amd import _lib
    geo = geos[kind]
    rows, bounds, acc = signed_cases(kind, n, 'events')
    what = '%s, %d photons, three rows, noise' % (kind, n)
    nrows = len(bounds) - 1
    (tx, ty, qx, qy), unit = daq_tables(geo)
    noise, count_cdf, accept = noise_tables(geo)
    kept = noise.sample(WINDOW, nrows, geo.nchannels, (qx, qy), unit, seed=SEED, acquisition=BASE)          # chroma_daq_noise_host
    assert len(kept) >= 60 and (kept['charge_int'] == 0).sum() >= 0.2 * len(kept) and (kept['charge_int'] > 0).sum() >= 0.2 * len(kept), what
    want = expected_with_noise(acc, kept, WINDOW, nrows, geo.nchannels)
    daq = tables_of(gpu, geo)
    dev = upload(rows)
    device_noise = Noise(count_cdf, accept)
    rc, naccepted = count_noise_rc(gpu, geo, daq, dev, bounds, WINDOW, device_noise)
    _lib.check(rc)
    assert naccepted == want['naccepted'], what
    out, row_noise = Outputs(nrows, naccepted), row_noise_words(nrows)
    rc, npulses = acquire_noise_rc(gpu, out, row_noise, geo, daq, dev, bounds, WINDOW, device_noise)
    _lib.check(rc)
    assert_pulses(out, npulses, want, what)
    assert_row_noise(row_noise, want['row_noise'], what)
    got = out.get()
    assert_sums_hold(got['q_int'][:npulses], got['npe'][:npulses].astype(np.uint64), max_count(geo), what)
