"""The dark noise of the time-binned DAQ without a GPU: the definition of include/chroma_hip.h ("dark noise") restated in NumPy,
the library's host twin (chroma_daq_noise_host) shown to BE that restatement bit for bit, the comparand of
tests/test_gpu_daq_noise.py built from the restated photons of tests/test_daq_pulses_host.py and the restated noise together, the
inputs of those tests shown to reach the edges they are there for, and ``gpu.DaqNoise``: its tables and its sampler.

The restatement loops over (row, channel): the words of Philox stream 1 + acquisition + row of the pseudo-photon
0xffffffff00000000 | channel (``oracle.philox``), the count from the integer table, per candidate the thinning, the bin from the
high word of b * nbins, the time in float32 with every operation rounded once, the charge as a photon's.  Everything is exact:
bits and integers.

The comparand.  ``expected_pulses`` of tests/test_daq_pulses_host.py bins every entry by its TIME; a noise photoelectron lies in
the bin it DREW, whatever rounding makes of its time (the header says so): where (float)bin + f rounds up to bin + 1 -- one
candidate in 256 at 65536 bins -- the two differ.  ``expected_with_noise`` is that function's reduction over the photons' bins by
time and the noise's drawn bins; where no noise time leaves its bin it is asserted to equal ``expected_pulses`` of photons and noise
together, and the windows of 65536 bins are asserted to hold a time that does leave.
"""
import numpy as np
import pytest

from chroma_amd import event
from test_gpu_photon_arrays import host_geos, daq_rows, daq_tables, DAQ_BASE, DAQ_FIRST, DAQ_N, DETECT          # noqa: F401
from test_gpu_daq_events import BASE
from test_daq_pulses_host import (uniform, interp_table, roundf, charge_count, restate, place, expected_pulses, time_image, time_bits, W_ALL, W_CUT,
                                  W_FINE, W_ONE, SEED, F)

WINDOWS = {'all': W_ALL, 'cut': W_CUT, 'one': W_ONE, 'fine': W_FINE}
NROWS = (1, 3, 70)
LEVELS = {'high': 2.5, 'low': 1e-3}          # mu of the channel with the largest rate
NOISE = event.DARK_NOISE
# the rates of the channels in units of the largest: zeros, the maximum, and fractions that thin
PATTERN = (1.0, 0.0, 0.5, 0.25, 1.0, 0.03125, 0.0, 0.75)
NOISE_DTYPE = [('row', np.int64), ('channel', np.int64), ('candidate', np.int64), ('bin', np.uint32), ('time', F), ('charge_int', np.uint32)]


def bounds_of(nrows):
    """1, 3 or 70 events over the window [DAQ_FIRST, DAQ_FIRST + DAQ_N) of ``daq_rows``, events without photons among them."""
    if nrows == 1:
        sizes = [DAQ_N]
    elif nrows == 3:
        sizes = [0, 1543, DAQ_N - 1543]
    else:
        sizes = np.random.default_rng(70).integers(0, 80, nrows)
        sizes[[0, 5, 6, 40, nrows - 1]] = 0
        sizes[20] = 300
    bounds = (DAQ_FIRST + np.cumsum(np.concatenate([[0], sizes]))).astype(np.uint32)
    assert len(bounds) == nrows + 1 and bounds[-1] <= DAQ_FIRST + DAQ_N
    return bounds


def noise_of(geo, window, level):
    """The DaqNoise whose largest rate gives ``LEVELS[level]`` candidates per word in ``window``: per-channel rates after PATTERN
    (one channel: the one rate)."""
    from chroma_amd.gpu.daq import DaqNoise
    top = LEVELS[level] / (1e-9 * window[2] * float(F(window[1])))
    if geo.nchannels == 1:
        return DaqNoise(top)
    return DaqNoise(top * np.resize(np.array(PATTERN), geo.nchannels))


# ---- the restatement -------------------------------------------------------------------------------------------------------
def restate_noise(oracle_mod, count_cdf, accept, tables, window, nrows, nchannels, base=BASE, seed=SEED):
    """(the kept noise photoelectrons in (row, channel, candidate) order, the candidates drawn, the candidates thinned away)"""
    (tx, ty, qx, qy), unit = tables
    unit = F(unit)
    t0, dt, nbins = F(window[0]), F(window[1]), int(window[2])
    key = (seed & 0xffffffff, seed >> 32)
    out = []
    drawn = thinned = 0
    for r in range(nrows):
        for c in range(nchannels):
            if accept[c] == 0:
                continue
            blocks = {}

            def word(w):
                if w >> 2 not in blocks:
                    blocks[w >> 2] = oracle_mod.philox((w >> 2, (1 + base + r) & 0xffffffff, c, 0xffffffff), key)
                return int(blocks[w >> 2][w & 3])
            k = int(sum(word(0) >= int(x) for x in count_cdf))
            drawn += k
            for j in range(k):
                a, b, d = word(1 + 3 * j), word(2 + 3 * j), word(3 + 3 * j)
                if not (a >> 1) < int(accept[c]):
                    thinned += 1
                    continue
                p = b * nbins
                bin_ = p >> 32
                f = F(F((p & 0xffffffff) >> 8) * F(2.0 ** -24))
                time = F(t0 + F(F(F(bin_) + f) * dt))
                charge = interp_table(uniform(d), qy, qx)
                out.append((r, c, j, bin_, time, charge_count(roundf(F(charge / unit)))))
    got = np.array(out, dtype=NOISE_DTYPE)
    got.flags.writeable = False
    return got, drawn, thinned


def expected_with_noise(acc, noise, window, nrows, nchannels, flag=NOISE):
    """What chroma_daq_acquire_pulses_noise returns for the accepted photons ``acc`` and the kept noise ``noise``: the dict of
    ``expected_pulses`` and row_noise (nrows).  The reduction is ``expected_pulses``'; the noise lies in its drawn bins."""
    nbins = int(window[2])
    inside, bins, early, late = place(acc, window)
    a = acc[inside]
    row = np.concatenate([a['row'], noise['row']])
    channel = np.concatenate([a['channel'], noise['channel']])
    keys = (row * nchannels + channel) * nbins + np.concatenate([bins[inside], noise['bin']]).astype(np.int64)
    charge = np.concatenate([a['charge_int'], noise['charge_int']]).astype(np.uint64)
    times = np.concatenate([a['time'], noise['time']]).astype(F)
    history = np.concatenate([a['history'], np.full(len(noise), flag, dtype=np.uint32)]).astype(np.uint32)
    unique, inverse = np.unique(keys, return_inverse=True)
    n = len(unique)
    q = np.zeros(n, dtype=np.uint64)
    np.add.at(q, inverse, charge)
    image = np.full(n, 0xffffffff, dtype=np.uint32)
    np.minimum.at(image, inverse, time_image(times.view(np.uint32)))
    flags = np.zeros(n, dtype=np.uint32)
    np.bitwise_or.at(flags, inverse, history)
    outside = np.zeros((nrows, 2), dtype=np.uint32)
    outside[:, 0] = np.bincount(acc['row'][early], minlength=nrows)
    outside[:, 1] = np.bincount(acc['row'][late], minlength=nrows)
    return dict(offsets=np.searchsorted(unique, np.arange(nrows + 1, dtype=np.int64) * nchannels * nbins).astype(np.uint32),
                channel=(unique // nbins % nchannels).astype(np.int32), bin=(unique % nbins).astype(np.uint32),
                npe=np.bincount(inverse, minlength=n).astype(np.uint32), q_int=(q & 0xffffffff).astype(np.uint32),
                t_first=time_bits(image), flags=flags, outside=outside.reshape(-1), naccepted=int(inside.sum()) + len(noise),
                row_noise=np.bincount(noise['row'], minlength=nrows).astype(np.uint32))


def as_accepted(acc, noise, flag=NOISE):
    """Photons and noise as one array of accepted photons, for ``expected_pulses``."""
    both = np.zeros(len(acc) + len(noise), dtype=acc.dtype)
    both[:len(acc)] = acc
    tail = both[len(acc):]
    tail['photon'], tail['row'], tail['channel'], tail['time'] = -1, noise['row'], noise['channel'], noise['time']
    tail['charge_int'], tail['history'] = noise['charge_int'], flag
    return both


def leaves_its_bin(noise, window):
    """The noise photoelectrons whose time, binned as a photon's is, does not give the drawn bin."""
    x = (noise['time'] - F(window[0])) / F(window[1])
    return ~((x >= F(0.0)) & (x < F(window[2])) & (np.floor(x) == noise['bin']))


@pytest.fixture(scope='module')
def noise_cases(oracle_mod, host_geos):
    """The cases of the CPU and of the GPU tests, restated once and shared read-only: noise_cases(which, nrows, window name, level)
    -> dict(rows, bounds, acc, noise (DaqNoise), count_cdf, accept, kept, drawn, thinned, want)."""
    photons, cache = {}, {}

    def get(which, nrows, wname, level):
        key = (which, nrows, wname, level)
        if key not in cache:
            geo = host_geos[which]
            if (which, nrows) not in photons:
                rows, bounds = daq_rows(geo), bounds_of(nrows)
                photons[which, nrows] = (rows, bounds, restate(oracle_mod, geo, rows[0], bounds))
            rows, bounds, acc = photons[which, nrows]
            window = WINDOWS[wname]
            noise = noise_of(geo, window, level)
            count_cdf, accept = noise.tables(window, geo.nchannels)
            kept, drawn, thinned = restate_noise(oracle_mod, count_cdf, accept, daq_tables(geo), window, nrows, geo.nchannels)
            cache[key] = dict(rows=rows, bounds=bounds, acc=acc, window=window, noise=noise, count_cdf=count_cdf, accept=accept, kept=kept,
                              drawn=drawn, thinned=thinned, want=expected_with_noise(acc, kept, window, nrows, geo.nchannels))
        return cache[key]
    return get


ALL_CASES = [(which, nrows, wname, level) for which in ('tiny', 'stress') for nrows in NROWS for wname in WINDOWS for level in LEVELS]


# ---- 1. the host twin is the restatement ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', ['tiny', 'stress'])
def test_the_host_twin_is_the_restatement(host_geos, noise_cases, which):
    geo = host_geos[which]
    (tx, ty, qx, qy), unit = daq_tables(geo)
    total = 0
    for _, nrows, wname, level in [c for c in ALL_CASES if c[0] == which]:
        case = noise_cases(which, nrows, wname, level)
        got = case['noise'].sample(case['window'], nrows, geo.nchannels, (qx, qy), unit, seed=SEED, acquisition=BASE)
        want = case['kept']
        what = '%s, %d rows, %s, %s' % (which, nrows, wname, level)
        assert len(got) == len(want), what
        for name in ('row', 'channel', 'bin', 'charge_int'):
            assert np.array_equal(got[name].astype(np.int64), want[name].astype(np.int64)), '%s: %s' % (what, name)
        assert np.array_equal(got['time'].view(np.uint32), want['time'].view(np.uint32)), what + ': time bits'
        assert (want['bin'] < case['window'][2]).all()
        total += len(want)
    assert total > (2000 if which == 'tiny' else 300)


def test_the_host_twin_refuses_what_the_header_says(host_geos):
    import ctypes
    from chroma_amd import _lib
    lib = _lib.load()
    geo = host_geos['tiny']
    (tx, ty, qx, qy), unit = daq_tables(geo)
    accept = np.full(geo.nchannels, 2 ** 31, dtype=np.uint32)
    good = np.array([2 ** 31, 2 ** 32 - 1], dtype=np.uint32)

    def rc(count_cdf=good, ncount=None, d_accept=accept, flag=NOISE, window=W_CUT, nrows=2, capacity=0):
        tables = _lib.DaqTables(None, None, 0, _lib.ptr(qx), _lib.ptr(qy), len(qx), unit)
        win = _lib.DaqWindow(*window)
        noise = _lib.DaqNoise(_lib.ptr(count_cdf), len(count_cdf) if ncount is None else ncount, _lib.ptr(d_accept), flag)
        n = ctypes.c_uint64(0)
        return lib.chroma_daq_noise_host(ctypes.byref(tables), ctypes.byref(win), ctypes.byref(noise), nrows, geo.nchannels, SEED, BASE,
                                         capacity, None, None, None, None, None, ctypes.byref(n)), int(n.value)
    code, n = rc()
    assert code == -1 and n > 0, 'no room: refused with the count'
    assert rc(ncount=0)[0] == -1 and rc(count_cdf=np.zeros(65, dtype=np.uint32))[0] == -1
    assert rc(count_cdf=np.array([5, 4], dtype=np.uint32))[0] == -1
    assert rc(flag=0)[0] == -1 and rc(flag=3)[0] == -1 and rc(flag=NOISE | DETECT)[0] == -1
    assert rc(count_cdf=None, ncount=2)[0] == -1 and rc(d_accept=None)[0] == -1
    assert rc(window=(0.0, 0.0, 5))[0] == -1 and rc(window=(0.0, 1.0, 65537))[0] == -1 and rc(nrows=0)[0] == -1
    assert rc(count_cdf=np.array([2 ** 32 - 1] * 64, dtype=np.uint32), d_accept=np.zeros(geo.nchannels, dtype=np.uint32)) == (0, 0)


# ---- 2. the comparand ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', ['tiny', 'stress'])
def test_the_comparand_is_expected_pulses_of_photons_and_noise_together(host_geos, noise_cases, which):
    """Where every noise time bins, as a photon's would, into the bin it drew, the comparand IS ``expected_pulses`` of the
    restated photons and the restated noise as one array; and in no other case is it, which is why it exists."""
    geo = host_geos[which]
    agree = differ = 0
    for _, nrows, wname, level in [c for c in ALL_CASES if c[0] == which]:
        case = noise_cases(which, nrows, wname, level)
        together = expected_pulses(as_accepted(case['acc'], case['kept']), case['window'], nrows, geo.nchannels)
        same = all(np.array_equal(together[name], case['want'][name]) for name in together)
        leaves = leaves_its_bin(case['kept'], case['window'])
        assert same == (not leaves.any()), '%s, %d rows, %s, %s' % (which, nrows, wname, level)
        agree += same
        differ += not same
        assert case['want']['row_noise'].sum() == len(case['kept'])
        assert case['want']['naccepted'] >= len(case['want']['npe'])
    assert agree >= 12 and (differ >= 1 or which == 'stress')


# ---- 3. the inputs exercise the edges --------------------------------------------------------------------------------------------
def test_the_cases_reach_the_edges_they_are_there_for(host_geos, noise_cases):
    geo = host_geos['tiny']
    nch = geo.nchannels
    accept = noise_cases('tiny', 70, 'one', 'high')['accept']
    assert (accept == 0).sum() >= 2 and (accept == 2 ** 31).sum() >= 2 and ((accept > 0) & (accept < 2 ** 31)).sum() >= 2
    for nrows in NROWS:
        assert (nrows * nch) % 256 != 0, 'the words of the chunk are a multiple of the block'
    assert 70 * nch > 8 * 256 and 3 * nch < 256, 'the words of 70 rows are one block of the noise kernels, or those of 3 rows more than a run'
    # a word with three or more kept candidates; candidates thinned away
    case = noise_cases('tiny', 70, 'one', 'high')
    kept = case['kept']
    per_word = np.bincount(kept['row'] * nch + kept['channel'], minlength=70 * nch)
    assert per_word.max() >= 3 and case['thinned'] > 50 and case['drawn'] == len(kept) + case['thinned']
    assert kept['candidate'].max() >= 4, 'no word reaches the second Philox block of its candidates'
    assert (per_word.reshape(70, nch)[:, accept == 0] == 0).all()
    # a pulse of light and noise; a pulse of two or more photoelectrons of noise alone
    want = case['want']
    assert ((want['flags'] & DETECT != 0) & (want['flags'] & NOISE != 0)).any(), 'no pulse mixes light and noise'
    assert ((want['flags'] == NOISE) & (want['npe'] >= 2)).any(), 'no pulse of two noise photoelectrons'
    assert ((want['flags'] & NOISE) == 0).any(), 'no pulse of light alone'
    # rows without photons have their noise
    bounds = case['bounds']
    empty = np.flatnonzero(np.diff(bounds.astype(np.int64)) == 0)
    assert len(empty) >= 3 and (want['row_noise'][empty] > 0).all() and (np.diff(want['offsets'].astype(np.int64))[empty] > 0).all()
    # the first and the last bin
    cut = noise_cases('tiny', 70, 'cut', 'high')['kept']
    assert cut['bin'].min() == 0 and cut['bin'].max() == W_CUT[2] - 1
    fine = noise_cases('tiny', 70, 'fine', 'high')
    assert fine['kept']['bin'].max() > 2 ** 15 and leaves_its_bin(fine['kept'], W_FINE).any(), 'no time rounds out of its drawn bin'
    # the low rate: some noise, and rows without any
    low = noise_cases('tiny', 70, 'all', 'low')
    assert 1 <= len(low['kept']) <= 20 and (low['want']['row_noise'] == 0).sum() >= 50, len(low['kept'])
    assert len(low['count_cdf']) <= 4 and len(case['count_cdf']) >= 12
    # the one-channel detector: every word is kept whole
    stress = noise_cases('stress', 70, 'all', 'high')
    assert stress['thinned'] == 0 and len(stress['kept']) > 100 and stress['accept'].tolist() == [2 ** 31]


TRIGGER = (3, 8)          # the trigger of the GPU tests: three channels within eight bins


def event_pulses_of(want, window, nchannels, unit):
    """The EventPulses of a comparand."""
    from chroma_amd.gpu.daq import EventPulses, DaqWindow
    return EventPulses(DaqWindow(*window), nchannels, unit, want['offsets'].astype(np.int64), want['channel'], want['bin'], want['npe'], want['q_int'],
                       want['t_first'].view(F), want['flags'], want['outside'].reshape(-1, 2), noise=want['row_noise'])


def test_noise_fires_triggers_that_light_alone_does_not(host_geos, noise_cases):
    """EventPulses.trigger (NumPy) on the comparand with and without the noise, 70 events, the window that holds everything."""
    geo = host_geos['tiny']
    unit = daq_tables(geo)[1]
    case = noise_cases('tiny', 70, 'all', 'high')
    light = expected_with_noise(case['acc'], case['kept'][:0], W_ALL, 70, geo.nchannels)
    assert not light['row_noise'].any() and all(np.array_equal(light[k], v) for k, v in expected_pulses(case['acc'], W_ALL, 70, geo.nchannels).items())
    with_noise = event_pulses_of(case['want'], W_ALL, geo.nchannels, unit).trigger(TRIGGER)
    without = event_pulses_of(light, W_ALL, geo.nchannels, unit).trigger(TRIGGER)
    assert len(without.bin) >= 5 and len(with_noise.bin) >= len(without.bin) + 5, (len(without.bin), len(with_noise.bin))
    empty = np.flatnonzero(np.diff(case['bounds'].astype(np.int64)) == 0)
    assert np.diff(with_noise.offsets)[empty].sum() >= 1, 'no event without photons fires on its noise'


# ---- 4. the tables ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mu', [1e-3, 0.5, 8.0])
def test_the_count_table_has_the_mean_of_the_poisson_distribution(mu):
    from math import exp, lgamma, log
    from chroma_amd.gpu.daq import DaqNoise, DaqWindow
    window = DaqWindow(0.0, 1.0, 1000)          # 1 us: a rate of mu MHz gives mu
    noise = DaqNoise(mu * 1e6)
    assert abs(noise.mu(window) - mu) < 1e-12 * mu
    count_cdf, accept = noise.tables(window, 3)
    n = len(count_cdf)
    assert count_cdf.dtype == np.uint32 and 1 <= n <= 64 and (np.diff(count_cdf.astype(np.int64)) >= 0).all()
    assert count_cdf[-1] == 2 ** 32 - 1 and (count_cdf[:-1] < 2 ** 32 - 1).all(), 'the table ends with its first saturated entry'
    mean = float(np.sum(2.0 ** 32 - count_cdf.astype(np.float64)) / 2.0 ** 32)          # E k = sum_j P(k > j)
    tail = sum(exp(-mu + j * log(mu) - lgamma(j + 1)) * (j - n + 1) for j in range(n, n + 200))          # sum_{j >= n} P(X > j)
    assert abs(mean - mu) <= n * 2.0 ** -32 + tail, (mean, mu, n, tail)
    assert accept.tolist() == [2 ** 31] * 3


def test_the_accept_words_and_what_daqnoise_refuses():
    from chroma_amd.gpu.daq import DaqNoise, DaqWindow
    window = DaqWindow(0.0, 1.0, 1000)
    count_cdf, accept = DaqNoise([0.0, 4000.0, 1000.0, 4000.0, 3.0]).tables(window, 5)
    assert accept.tolist() == [0, 2 ** 31, 2 ** 29, 2 ** 31, int(np.floor(3.0 / 4000.0 * 2.0 ** 31 + 0.5))]
    assert np.array_equal(count_cdf, DaqNoise(4000.0).tables(window, 1)[0])
    # the documented limit of a table of 64 entries
    assert len(DaqNoise(DaqNoise.MAX_MU * 1e6).tables(window, 1)[0]) == 64
    for mu in (26.0, 40.0, 1e3):
        with pytest.raises(ValueError):
            DaqNoise(mu * 1e6).tables(window, 1)
    for bad in (-1.0, float('nan'), float('inf'), [1.0, -2.0], [[1.0]], []):
        with pytest.raises(ValueError):
            DaqNoise(bad)
    for flag in (0, 3, 2 ** 32, 1.5):
        with pytest.raises(ValueError):
            DaqNoise(1.0, flag=flag)
    with pytest.raises(ValueError):
        DaqNoise([1.0, 2.0]).tables(window, 3)
    off = DaqNoise([0.0, 0.0])
    assert off.off and not DaqNoise(1.0).off and DaqNoise(1.0).flag == event.DARK_NOISE == 1 << 12
    assert len(off.sample(window, 4, 2, ([0.0, 1.0], [0.0, 1.0]), 0.5)) == 0
    noise = DaqNoise(5.0)
    assert DaqNoise.of(noise) is noise and DaqNoise.of(7.0).rate_hz == 7.0


# ---- 5. the sampler's statistics ---------------------------------------------------------------------------------------------------
def test_the_sampler_draws_poisson_counts_uniformly_over_the_window():
    """200 rows x 64 channels at mu = 0.5, a fixed seed: the total within 5 sigma of 6400, each of 8 bins within 5 sigma of 800."""
    from chroma_amd.gpu.daq import DaqNoise, DaqWindow
    window = DaqWindow(-20.0, 12.5, 8)          # 100 ns
    nrows, nch, mu = 200, 64, 0.5
    noise = DaqNoise(mu / (1e-9 * 100.0))
    got = noise.sample(window, nrows, nch, (np.array([0.0, 1.0, 2.0], dtype=F), np.array([0.0, 0.5, 1.0], dtype=F)), 2.0 / 2 ** 16, seed=2024)
    expect = nrows * nch * mu
    assert abs(len(got) - expect) <= 5.0 * np.sqrt(expect), len(got)
    occupancy = np.bincount(got['bin'], minlength=8)
    assert len(occupancy) == 8 and (np.abs(occupancy - expect / 8) <= 5.0 * np.sqrt(expect / 8)).all(), occupancy
    per_word = np.bincount(got['row'] * nch + got['channel'], minlength=nrows * nch)
    assert abs((per_word == 0).mean() - np.exp(-mu)) <= 5.0 * np.sqrt(np.exp(-mu) * (1 - np.exp(-mu)) / (nrows * nch))
    edges = window.bin_edges()
    assert (got['time'] >= edges[got['bin']]).all() and (got['time'] <= edges[got['bin'] + 1]).all()
    assert got['charge_int'].min() >= 0 and got['charge_int'].max() <= 2 ** 16 and len(np.unique(got['charge_int'])) > 1000
    # a row is its own stream: the rows of a later call are the rows of this one
    again = noise.sample(window, 50, nch, (np.array([0.0, 1.0, 2.0], dtype=F), np.array([0.0, 0.5, 1.0], dtype=F)), 2.0 / 2 ** 16, seed=2024, acquisition=150)
    tail = got[got['row'] >= 150]
    assert len(again) == len(tail) and np.array_equal(again['row'] + 150, tail['row'])
    assert all(np.array_equal(again[name], tail[name]) for name in ('channel', 'bin', 'charge_int')) and np.array_equal(again['time'].view(np.uint32), tail['time'].view(np.uint32))


def test_chroma_sim_wants_a_window_and_a_rate_that_is_one():
    from chroma_amd import cli
    for argv in (['@chroma_amd.demo.tiny', '--daq-noise', '1000'], ['@chroma_amd.demo.tiny', '--daq-window=-8,0.5,512', '--daq-noise=-5'],
                 ['@chroma_amd.demo.tiny', '--daq-window=-8,0.5,512', '--daq-noise', 'inf']):
        with pytest.raises(SystemExit):
            cli.main(argv)
