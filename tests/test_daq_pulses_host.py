"""The time-binned DAQ without a GPU: the comparand of tests/test_gpu_daq_pulses.py, its inputs, and EventPulses.

The comparand is a NumPy restatement of what k_run_daq_events (and so the pulses' emit) does per photon -- the rejects, the three
draws of Philox stream 1 + acquisition + row (``oracle.philox``, words 0 to 2), cm_u32_to_uniform, interp_table and roundf in
float32 -- then the binning of include/chroma_hip.h in float32 and ``np.unique`` over (row, channel, bin).  Here it is first
shown to BE the oracle's DAQ: reduced per (row, channel) the way run_daq reduces (unsigned minimum of the time bits against the
reset value, sum, OR) it gives ``oracle_rows`` word for word.  Then the windows and inputs of the GPU tests are shown to reach
the edges they are there for.  Everything is exact: bits and integers.
"""
import numpy as np
import pytest

from chroma_amd import event
from test_gpu_photon_arrays import host_geos, daq_rows, daq_tables, DAQ_BASE, DAQ_FIRST, DAQ_N, DETECT          # noqa: F401
from test_gpu_daq_events import event_bounds, many_rows_and_bounds, oracle_rows, BASE, WEIGHT, RESET_BITS

F = np.float32
SEED = 9

# ---- the windows of the GPU tests (t0, dt, nbins) --------------------------------------------------------------------------
W_ALL = (-64.0, 0.25, 512)            # holds every accepted time
W_CUT = (-1.0, 0.5, 5)                # early and late photons, rows without a pulse
W_FINE = (-4.0, 2.0 ** -13, 65536)    # the most bins there are: bins above 2^15
W_ONE = (-64.0, 128.0, 1)             # one bin: a key per (row, channel)


# ---- the restatement -------------------------------------------------------------------------------------------------------
def uniform(word):
    """cm_u32_to_uniform"""
    return F(F(F(word) * F(2.3283064365386963e-10)) + F(1.1641532182693481e-10))


def interp_table(x, xp, fp):
    """interp_table of device_common.h (interpolate.h:32-57) in float32, each operation rounded once."""
    lower, upper = 0, len(xp) - 1
    if x <= xp[lower]:
        return fp[lower]
    if x >= xp[upper]:
        return fp[upper]
    while lower < upper - 1:
        half = (lower + upper) // 2
        if x < xp[half]:
            upper = half
        else:
            lower = half
    df = F(fp[upper] - fp[lower])
    dx = F(xp[upper] - xp[lower])
    return F(fp[lower] + F(F(df * F(x - xp[lower])) / dx))


def roundf(x):
    """roundf: to the nearest integer, halves away from zero (exact: the fraction of a float32 below 2^23 is a float32)"""
    r = np.trunc(x)
    if abs(F(x - r)) >= F(0.5):
        r = r + np.sign(x)
    return F(r)


def charge_count(x):
    """float -> uint32 as the DAQ counts a charge (cvt.rzi.u32.f32 / v_cvt_u32_f32), in Python integers: toward zero; NaN and
    negatives give 0; saturating."""
    x = float(x)
    if x != x or x < 0.0:
        return 0
    if x > float(2 ** 32 - 1):
        return 2 ** 32 - 1
    return min(max(int(x), 0), 2 ** 32 - 1)


def restate(oracle_mod, geo, ph, bounds, base=BASE, weight=WEIGHT, seed=SEED, id_base=DAQ_BASE, signed=False):
    """The accepted photons of the rows of ``bounds`` in photon order: a structured array of (photon, row, channel, time,
    charge_int, history).  ``signed``: the detector's charge CDF starts below zero (tests/signed_charge.py)."""
    (tx, ty, qx, qy), unit = daq_tables(geo)
    unit, weight = F(unit), F(weight)
    key = (seed & 0xffffffff, seed >> 32)
    out = []
    for r in range(len(bounds) - 1):
        for i in range(int(bounds[r]), int(bounds[r + 1])):
            triangle = int(ph.last_hit_triangles[i])
            if triangle <= -1:
                continue
            channel = int(geo.channel_of_triangle[triangle])
            history = int(ph.flags[i])
            if channel < 0 or not history & DETECT:
                continue
            pid = id_base + i
            words = oracle_mod.philox((0, (1 + base + r) & 0xffffffff, pid & 0xffffffff, pid >> 32), key)
            if not uniform(words[0]) < F(ph.weights[i] * weight):
                continue
            time = F(ph.t[i] + interp_table(uniform(words[1]), ty, tx))
            charge = interp_table(uniform(words[2]), qy, qx)
            assert charge >= 0 or signed
            out.append((i, r, channel, time, charge_count(roundf(F(charge / unit))), history, charge))
    dtype = [('photon', np.int64), ('row', np.int64), ('channel', np.int64), ('time', F), ('charge_int', np.uint32), ('history', np.uint32),
             ('charge', F)]
    acc = np.array(out, dtype=dtype)
    acc.flags.writeable = False
    return acc


def place(acc, window):
    """(in the window, bin, early, late) of the accepted photons: the binning of include/chroma_hip.h in float32."""
    t0, dt, nbins = F(window[0]), F(window[1]), int(window[2])
    x = (acc['time'] - t0) / dt
    assert x.dtype == F
    inside = (x >= F(0.0)) & (x < F(nbins))
    bins = np.floor(np.where(inside, x, F(0.0))).astype(np.uint32)
    early = ~inside & (acc['time'] < t0)
    return inside, bins, early, ~inside & ~early


def time_image(bits):
    """The order-preserving image of float bits: a < b as floats <=> image(a) < image(b) as unsigned (-0 below +0)."""
    bits = np.asarray(bits, dtype=np.uint32)
    return np.where(bits >> 31 != 0, ~bits, bits | np.uint32(0x80000000)).astype(np.uint32)


def time_bits(image):
    image = np.asarray(image, dtype=np.uint32)
    return np.where(image >> 31 != 0, image & np.uint32(0x7fffffff), ~image).astype(np.uint32)


def expected_pulses(acc, window, nrows, nchannels):
    """What chroma_daq_acquire_pulses returns for the accepted photons ``acc``: a dict of offsets (nrows + 1), channel, bin,
    npe, q_int, t_first (bits), flags, outside (2 * nrows) and naccepted."""
    nbins = int(window[2])
    inside, bins, early, late = place(acc, window)
    a = acc[inside]
    keys = (a['row'] * nchannels + a['channel']) * nbins + bins[inside].astype(np.int64)
    unique, inverse = np.unique(keys, return_inverse=True)
    n = len(unique)
    q = np.zeros(n, dtype=np.uint64)
    np.add.at(q, inverse, a['charge_int'].astype(np.uint64))
    image = np.full(n, 0xffffffff, dtype=np.uint32)
    np.minimum.at(image, inverse, time_image(a['time'].view(np.uint32)))
    flags = np.zeros(n, dtype=np.uint32)
    np.bitwise_or.at(flags, inverse, a['history'])
    outside = np.zeros((nrows, 2), dtype=np.uint32)
    outside[:, 0] = np.bincount(acc['row'][early], minlength=nrows)
    outside[:, 1] = np.bincount(acc['row'][late], minlength=nrows)
    return dict(offsets=np.searchsorted(unique, np.arange(nrows + 1, dtype=np.int64) * nchannels * nbins).astype(np.uint32),
                channel=(unique // nbins % nchannels).astype(np.int32), bin=(unique % nbins).astype(np.uint32),
                npe=np.bincount(inverse, minlength=n).astype(np.uint32), q_int=(q & 0xffffffff).astype(np.uint32),
                t_first=time_bits(image), flags=flags, outside=outside.reshape(-1), naccepted=int(inside.sum()))


def edge_windows(acc):
    """The two windows cut to the accepted photons ``acc``: (t0 on photon a's time: a is in bin 0; one bin from there of the
    width float32(t_b - t0): b has x == 1.0 and is late), and the photons a and b (indices into ``acc``)."""
    order = np.argsort(acc['time'], kind='stable')
    a = order[len(order) // 2]
    t0 = acc['time'][a]
    later = order[acc['time'][order] > t0 + F(0.1)]
    b = later[0]
    return (float(t0), 0.5, 16), (float(t0), float(F(acc['time'][b] - t0)), 1), a, b


@pytest.fixture(scope='module')
def restated(oracle_mod, host_geos):
    """The accepted photons, restated once per case and shared read-only: restated(which, kind) -> (rows, bounds, acc) with kind
    'events' (daq_rows under event_bounds), 'many' (many_rows_and_bounds) or 'whole' (daq_rows, every photon of the set, guard
    photons included, as ONE event)."""
    cache = {}

    def get(which, kind='events'):
        if (which, kind) not in cache:
            geo = host_geos[which]
            if kind == 'many':
                rows, bounds = many_rows_and_bounds(geo)
            else:
                rows = daq_rows(geo)
                bounds = event_bounds() if kind == 'events' else np.array([0, len(rows[0])], dtype=np.uint32)
            cache[which, kind] = (rows, bounds, restate(oracle_mod, geo, rows[0], bounds))
        return cache[which, kind]
    return get


# ---- 1. the restatement is the oracle's DAQ ----------------------------------------------------------------------------------
@pytest.mark.parametrize('which', ['tiny', 'stress'])
def test_the_restatement_is_the_oracles_daq(oracle_mod, host_geos, restated, which):
    geo = host_geos[which]
    rows, bounds, acc = restated(which)
    nrows, nch = len(bounds) - 1, geo.nchannels
    state = oracle_rows(oracle_mod, geo, rows[0], bounds)
    word = acc['row'] * nch + acc['channel']
    t = np.full(nrows * nch, RESET_BITS, dtype=np.uint32)
    np.minimum.at(t, word, acc['time'].view(np.uint32))
    q = np.zeros(nrows * nch, dtype=np.uint64)
    np.add.at(q, word, acc['charge_int'].astype(np.uint64))
    hist = np.zeros(nrows * nch, dtype=np.uint32)
    np.bitwise_or.at(hist, word, acc['history'])
    assert len(acc) > 300
    assert np.array_equal(t, state[0]), 'time bits'
    assert np.array_equal((q & 0xffffffff).astype(np.uint32), state[1]), 'charge counts'
    assert np.array_equal(hist, state[2]), 'histories'


def test_the_restatement_is_the_oracles_daq_on_the_many_events(oracle_mod, host_geos, restated):
    geo = host_geos['tiny']
    rows, bounds, acc = restated('tiny', 'many')
    state = oracle_rows(oracle_mod, geo, rows[0], bounds)
    word = acc['row'] * geo.nchannels + acc['channel']
    hist = np.zeros(len(state[2]), dtype=np.uint32)
    np.bitwise_or.at(hist, word, acc['history'])
    q = np.zeros(len(state[1]), dtype=np.uint64)
    np.add.at(q, word, acc['charge_int'].astype(np.uint64))
    assert np.array_equal(hist, state[2]) and np.array_equal(q.astype(np.uint32), state[1])


# ---- 2. the inputs exercise the edges ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', ['tiny', 'stress'])
def test_the_windows_reach_their_edges(host_geos, restated, which):
    geo = host_geos[which]
    rows, bounds, acc = restated(which)
    nrows, nch = len(bounds) - 1, geo.nchannels
    # the window that holds everything
    inside, bins, early, late = place(acc, W_ALL)
    assert inside.all() and not early.any() and not late.any()
    everything = expected_pulses(acc, W_ALL, nrows, nch)
    assert everything['naccepted'] == len(acc) and (everything['npe'] >= 2).any(), 'no bin with two photoelectrons'
    # the cut: early and late photons in several rows, rows without a pulse
    cut = expected_pulses(acc, W_CUT, nrows, nch)
    outside = cut['outside'].reshape(nrows, 2)
    assert (outside[:, 0] > 0).sum() >= 3 and (outside[:, 1] > 0).sum() >= 3
    assert (np.diff(cut['offsets'].astype(np.int64)) == 0).sum() >= 3 and 0 < cut['naccepted'] < len(acc)
    assert cut['bin'].max() == 4 and cut['bin'].min() == 0
    # t0 on a photon's own time: bin 0; one bin of the width to another photon: that one is late, x == 1.0
    on_a, to_b, a, b = edge_windows(acc)
    inside, bins, early, late = place(acc, on_a)
    assert inside[a] and bins[a] == 0
    inside, bins, early, late = place(acc, to_b)
    x = (acc['time'][b] - F(to_b[0])) / F(to_b[1])
    assert x == F(1.0) and late[b] and not inside[b] and inside[a] and inside.sum() >= 1
    # the most bins
    fine = expected_pulses(acc, W_FINE, nrows, nch)
    assert fine['bin'].max() > 2 ** 15 and fine['naccepted'] > 100
    if which == 'tiny':
        # the first channel's photons are 30 to 40 ns early: negative times only
        first = everything['channel'] == np.unique(geo.channel_of_triangle[geo.on])[0]
        assert first.sum() >= 3 and (everything['t_first'][first].view(F) < 0).all()
        assert (everything['t_first'].view(F) > 0).any()


def test_one_key_runs_over_many_waves(host_geos, restated):
    """'stress' (one channel), every photon of the set as ONE event, one bin: one key, and its run is longer than 512."""
    rows, bounds, acc = restated('stress', 'whole')
    want = expected_pulses(acc, W_ONE, 1, 1)
    assert len(want['npe']) == 1 and want['naccepted'] == len(acc)
    assert want['npe'][0] > 512, 'the run of the one key is %d photons' % want['npe'][0]


@pytest.mark.parametrize('which', ['tiny', 'stress'])
def test_one_event_of_every_photon_has_early_and_late_photons_in_every_wave(host_geos, restated, which):
    """The whole set as one event under the window that cuts: more than three blocks of 1024 photons, all of one row, and more
    early and more late photons than a wave is lanes."""
    rows, bounds, acc = restated(which, 'whole')
    want = expected_pulses(acc, W_CUT, 1, host_geos[which].nchannels)
    assert len(rows[0]) > 3 * 1024 and want['outside'][0] > 64 and want['outside'][1] > 64 and want['naccepted'] > 64


def test_the_many_events_have_rows_without_pulses_and_pulses_in_the_first_and_the_last(host_geos, restated):
    geo = host_geos['tiny']
    rows, bounds, acc = restated('tiny', 'many')
    nrows = len(bounds) - 1
    want = expected_pulses(acc, W_ALL, nrows, geo.nchannels)
    sizes = np.diff(want['offsets'].astype(np.int64))
    assert sizes[0] > 0 and sizes[-1] > 0 and (sizes == 0).sum() > 100 and nrows * geo.nchannels > 2 ** 16
    assert want['channel'][0] == 0 and want['channel'][-1] == geo.nchannels - 1


# ---- 3. EventPulses on hand-made arrays ------------------------------------------------------------------------------------------
def handmade():
    from chroma_amd.gpu.daq import EventPulses, DaqWindow
    window = DaqWindow(-1.0, 0.5, 6)
    # three events: two pulses on channel 1 and one on channel 3; none; one on channel 0
    offsets = np.array([0, 3, 3, 4], dtype=np.int64)
    channel = np.array([1, 1, 3, 0], dtype=np.int32)
    bins = np.array([0, 5, 2, 4], dtype=np.uint32)
    npe = np.array([2, 1, 7, 1], dtype=np.uint32)
    q_int = np.array([100, 40, 700, 65536], dtype=np.uint32)
    t_first = np.array([-0.9, 1.6, 0.1, 1.2], dtype=F)
    flags = np.array([4, 4, 6, 4], dtype=np.uint32)
    outside = np.array([[1, 2], [0, 0], [0, 9]], dtype=np.uint32)
    return EventPulses(window, 4, 0.25, offsets, channel, bins, npe, q_int, t_first, flags, outside), window


def test_event_pulses_slices_outside_and_waveform():
    pulses, window = handmade()
    assert len(pulses) == 3 and pulses.window is window and pulses.nchannels == 4
    assert np.array_equal(pulses.bin_edges(), [-1.0, -0.5, 0.0, 0.5, 1.0, 1.5, 2.0]) and np.array_equal(window.bin_edges(), pulses.bin_edges())
    channel, bins, npe, q, t_first, flags = pulses.sparse(0)
    assert channel.tolist() == [1, 1, 3] and bins.tolist() == [0, 5, 2] and npe.tolist() == [2, 1, 7] and flags.tolist() == [4, 4, 6]
    assert q.dtype == F and np.array_equal(q, (np.array([100, 40, 700]).astype(F) * F(0.25)).astype(F)) and t_first.tolist() == [F(-0.9), F(1.6), F(0.1)]
    assert channel.base is not None, 'sparse() returns slices, not copies'
    assert np.array_equal(pulses.q_int, [100, 40, 700, 65536]) and pulses.q[3] == F(16384.0)
    assert pulses.outside(0) == (1, 2) and pulses.outside(1) == (0, 0) and pulses.outside(2) == (0, 9)
    npe, q = pulses.waveform(0, 1)
    assert npe.dtype == np.uint32 and q.dtype == F and npe.tolist() == [2, 0, 0, 0, 0, 1] and q.tolist() == [25.0, 0, 0, 0, 0, 10.0]
    npe, q = pulses.waveform(0, 3)
    assert npe.tolist() == [0, 0, 7, 0, 0, 0] and q.tolist() == [0, 0, 175.0, 0, 0, 0]
    for channel in (0, 2):
        npe, q = pulses.waveform(0, channel)
        assert not npe.any() and not q.any() and len(npe) == len(q) == 6


def test_event_pulses_empty_events_negative_and_bad_indices():
    pulses, window = handmade()
    assert all(len(a) == 0 for a in pulses.sparse(1))
    npe, q = pulses.waveform(1, 2)
    assert len(npe) == 6 and not npe.any() and not q.any()
    assert pulses.sparse(-1)[0].tolist() == [0] and pulses.sparse(-3)[0].tolist() == [1, 1, 3] and pulses.outside(-1) == (0, 9)
    assert pulses.waveform(-1, 0)[0].tolist() == [0, 0, 0, 0, 1, 0]
    one = pulses.event(-1)
    assert len(one) == 1 and one.window is window and (one.early, one.late) == (0, 9) and one.q_int.tolist() == [65536]
    assert len(pulses.event(1)) == 0
    for i in (3, -4, 100):
        with pytest.raises(IndexError):
            pulses.sparse(i)
        with pytest.raises(IndexError):
            pulses.outside(i)
        with pytest.raises(IndexError):
            pulses.waveform(i, 0)
    for channel in (4, -1):
        with pytest.raises(IndexError):
            pulses.waveform(0, channel)
    assert event.Event().pulses is None


def test_a_window_that_is_none_is_refused():
    from chroma_amd.gpu.daq import DaqWindow
    for bad in ((0.0, 0.0, 5), (0.0, -1.0, 5), (0.0, float('nan'), 5), (float('inf'), 1.0, 5), (0.0, 1.0, 0), (0.0, 1.0, 65537), (0.0, 1.0, 2.5),
                (0.0, 1.0), 'soon'):
        with pytest.raises(ValueError):
            DaqWindow.of(bad)
    w = DaqWindow.of((0.0, 1.0, 65536))
    assert DaqWindow.of(w) is w and w == DaqWindow(0.0, 1.0, 65536) and w.nbins == 65536
