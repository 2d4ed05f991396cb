"""The digitiser of the time-binned DAQ on the host: chroma_daq_digitize_host (daq_digitize_host.cpp, the plain-loop twin of
chroma_daq_digitize_gates) and EventTriggers.digitize over it, against a brute-force restatement of the definition in
include/chroma_hip.h ("digitiser") -- Python integers over hit, sample and pulse, its own Philox (oracle.philox) -- which shares
no code with the package.  Every sample and every flag word is compared exactly.

The pulse sets are those of tests/test_daq_trigger_host.py with their triggers (gates of 1 .. 200 samples, windows of 1 .. 65 536
bins, firings at bin 0 and in the last bin: traces reach before the window and beyond it), each under several digitisers, and
hand-made sets for the edges of the definition.  tests/test_gpu_daq_digitize.py runs the same through the device call.
"""
import ctypes
import functools

import numpy as np
import pytest

from test_daq_trigger_host import cases, brute, brute_of, from_rows, PulseSet

ERR_INVALID = -1
CHARGE_UNIT = 0.125          # (PulseSet.event_pulses')
SEED, ACQUISITION = 0x1234567887654321, 0xfffffffe          # (the streams 1 + acquisition + row wrap within a set)
NOISE_LO = -32


class Digitiser(object):
    """A chroma_daq_digitizer as integers: taps, shift, pedestal, bits, and sigma (0: no noise) for the table."""

    def __init__(self, name, taps, shift, pedestal, bits, sigma=0.0):
        self.name, self.taps, self.shift, self.pedestal, self.bits, self.sigma = name, np.asarray(taps, dtype=np.int32), shift, pedestal, bits, sigma
        self.noise_cdf = noise_table(sigma) if sigma else np.zeros(0, dtype=np.uint32)

    def struct(self, **change):
        from chroma_amd import _lib
        v = dict(taps=_lib.ptr(self.taps), ntaps=len(self.taps), shift=self.shift, pedestal=self.pedestal, bits=self.bits,
                 noise_cdf=_lib.ptr(self.noise_cdf) if len(self.noise_cdf) else None, nnoise=len(self.noise_cdf), noise_lo=NOISE_LO)
        v.update(change)
        return _lib.DaqDigitizer(*[v[k] for k in ('taps', 'ntaps', 'shift', 'pedestal', 'bits', 'noise_cdf', 'nnoise', 'noise_lo')])

    def of_the_package(self):
        """The gpu.DaqDigitizer whose tables for CHARGE_UNIT are these integers (powers of two: exact)."""
        from chroma_amd.gpu.daq import DaqDigitizer
        return DaqDigitizer(self.taps.astype(np.float64) / (CHARGE_UNIT * 2.0 ** self.shift), pedestal=self.pedestal, bits=self.bits, shift=self.shift,
                            noise_sigma=self.sigma)


def noise_table(sigma):
    """The header's: entry j = floor(Phi((noise_lo + j + 0.5) / sigma) * 2^32) in float64, saturated."""
    import math
    return np.array([min(int(math.floor(0.5 * (1.0 + math.erf((NOISE_LO + j + 0.5) / sigma / math.sqrt(2.0))) * 2.0 ** 32)), 0xffffffff) for j in range(64)],
                    dtype=np.uint32)


@functools.lru_cache(maxsize=None)
def digitisers():
    """ntaps 1, 2, 64, 65 and 1024; negative taps; 1 and 16 bits; with and without noise.  The charge counts of the sets span
    2^13 .. 2^32, so the gains are small: some samples stay inside the range, some clip."""
    rng = np.random.default_rng(31)
    d = np.arange(1024, dtype=np.float64)
    return [Digitiser('1 tap', [1 << 21], 31, 100, 14),
            Digitiser('2 taps, one negative, noise', [3 << 16, -(5 << 15)], 30, 2000, 12, 1.5),
            Digitiser('64 taps of both signs, 16 bits', rng.integers(-(1 << 12), 1 << 12, 64), 28, 30000, 16),
            Digitiser('65 taps, 1 bit, noise of sigma 8', np.rint(4096.0 * np.exp(-d[:65] / 20.0)), 31, -3, 1, 8.0),
            Digitiser('1024 taps with an undershoot, noise', np.rint(60000.0 * np.exp(-d / 6.0) - 900.0 * np.exp(-d / 300.0)), 31, 300, 10, 0.7)]


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def philox_word(blocks, seed, stream, channel, u):
    import oracle
    key = (int(seed) & 0xffffffff, int(seed) >> 32)
    at = (stream, channel, u >> 2)
    if at not in blocks:
        blocks[at] = oracle.philox((0x80000000 | (u >> 2), stream, channel & 0xffffffff, 0xffffffff), key)
    return int(blocks[at][u & 3])


def brute_adc(ps, trig, want, dig, seed=SEED, acquisition=ACQUISITION):
    """(adc[nhits][G] uint16, trace_flags[nhits] uint32) of the hits of `want` (a brute-force trigger result on `ps`)."""
    threshold, W, H, pre, post = trig
    G = pre + post
    taps, ntaps = [int(t) for t in dig.taps], len(dig.taps)
    cdf = [int(x) for x in dig.noise_cdf]
    top = (1 << dig.bits) - 1
    nhits = len(want['hit_channel'])
    adc, flags = np.zeros((nhits, G), dtype=np.uint16), np.zeros(nhits, dtype=np.uint32)
    blocks = {}
    for r in range(ps.nrows):
        lo, hi = int(ps.offsets[r]), int(ps.offsets[r + 1])
        for k in range(int(want['trig_offsets'][r]), int(want['trig_offsets'][r + 1])):
            b = int(want['trig_bin'][k])
            for i in range(int(want['hit_offsets'][k]), int(want['hit_offsets'][k + 1])):
                c = int(want['hit_channel'][i])
                mine = [(int(ps.bin[p]), int(ps.q_int[p])) for p in range(lo, hi) if ps.channel[p] == c]
                for s in range(G):
                    B = b - pre + s
                    acc = 0
                    for p_bin, q in mine:
                        if 0 <= B - p_bin < ntaps:
                            acc = (acc + ((q * taps[B - p_bin]) & 0xffffffffffffffff)) & 0xffffffffffffffff
                    if acc >= 1 << 63:
                        acc -= 1 << 64
                    e = 0
                    if cdf:
                        w = philox_word(blocks, seed, (1 + acquisition + r) & 0xffffffff, c, B + 65536)
                        e = NOISE_LO + sum(w >= x for x in cdf)
                    v = dig.pedestal + (acc >> dig.shift) + e
                    if v > top:
                        v, flags[i] = top, flags[i] | 1
                    elif v < 0:
                        v, flags[i] = 0, flags[i] | 2
                    adc[i, s] = v
    return adc, flags


@functools.lru_cache(maxsize=None)
def brute_traces(index, which):
    name, ps, trig = cases()[index]
    return brute_adc(ps, trig, brute(index, 'nhit'), digitisers()[which])


def handmade():
    """[(name, PulseSet, trigger, Digitiser)]: the edges of the definition, one set each."""
    rng = np.random.default_rng(12)
    out = []
    # firing at 20 (two channels in one bin), pre 2: sample 0 is bin 18.  Five taps: channel 0's pulse in bin 14 is ntaps - 1 bins
    # before and counts, channel 1's in bin 13 is ntaps before and does not
    ps = from_rows(1, 2, 40, [{(0, 14), (0, 20), (1, 13), (1, 20)}], rng)
    ps.q_int[:] = [1000, 3, 1000, 3]
    out.append(('reach of the taps', ps, (2, 1, 8, 2, 6), Digitiser('five taps', [1 << 8, 0, 0, 0, 1 << 4], 8, 7, 14)))
    # firings at 20 and 26, gates [18, 24) and [24, 30): the pulse in bin 22 lies in the first gate, its tail in the second trace
    ps = from_rows(1, 1, 40, [{(0, 20), (0, 22), (0, 26), (0, 27)}], rng)
    ps.q_int[:] = [100, 5000, 10, 20]
    out.append(('tail from the gate before', ps, (1, 1, 6, 2, 4), Digitiser('eight taps', [256 >> d for d in range(8)], 8, 0, 14)))
    # 150 pulses in consecutive bins under 100 taps: more than one wave-load of pulses reaches one sample; the gate of 200
    # samples from bin 10 on runs beyond the window of 200 bins
    ps = from_rows(1, 2, 200, [{(1, b) for b in range(10, 160)}], rng)
    ps.q_int[:] = rng.integers(1, 1000, 150)
    out.append(('150 pulses under 100 taps', ps, (1, 1, 200, 0, 200), Digitiser('100 taps', rng.integers(-50, 400, 100), 10, 50, 16)))
    # saturation.  Firing at 10 (channels 0 and 3, no charge), gate [8, 16); taps +, - twice as large.  Channel 1: a large pulse in
    # the gate's last bin, the top alone; channel 2: one in bin 7, before the gate, whose negative tap is sample 0, and an empty one
    # in the gate: 0 alone; channel 4: one in bin 11, both; channels 0 and 3: neither
    ps = from_rows(1, 5, 40, [{(0, 10), (3, 10), (1, 15), (2, 7), (2, 12), (4, 11)}], rng)
    ps.q_int[:] = [0, 1 << 20, 1 << 20, 0, 0, 1 << 20]          # (in (channel, bin) order)
    out.append(('saturation', ps, (2, 1, 8, 2, 6), Digitiser('up and down', [1 << 4, -(1 << 5)], 8, 100, 12)))
    # the 64-bit sum wraps: charge counts of 2^32 - 1 on taps of -2^31, three pulses in reach of one sample
    ps = from_rows(1, 1, 40, [{(0, 10), (0, 11), (0, 12)}], rng)
    ps.q_int[:] = 0xffffffff
    out.append(('the sum wraps', ps, (1, 1, 8, 2, 6), Digitiser('three taps of -2^31', [-(1 << 31)] * 3, 0, 0, 16)))
    # a trigger without hits (the sum of bin 5 is still up when the lockout ends at 8, where the gate holds nothing) and a row
    # without pulses
    ps = from_rows(3, 2, 30, [{(0, 5)}, set(), {(1, 3), (0, 3)}], rng)
    ps.q_int[:] = [700, 800, 900]
    out.append(('a trigger without hits', ps, (1, 10, 3, 0, 1), Digitiser('two taps, noise', [1 << 8, 1 << 7], 8, 10, 14, 3.0)))
    return out


@functools.lru_cache(maxsize=None)
def handmade_results():
    out = []
    for name, ps, trig, dig in handmade():
        want = brute_of(ps, 'nhit', *trig)
        out.append((want,) + brute_adc(ps, trig, want, dig))
    return out


# ---- the calls -------------------------------------------------------------------------------------------------------------------------
def call_arguments(ps, trig, want, dig_struct, seed, acquisition, first_hit, nhits_call, capacity, adc, flags, change=None):
    """The arguments of both calls behind the context: (nrows, nchannels, window, trigger, digitizer, ..., adc, trace_flags), host
    arrays as numpy arrays (the caller turns them into pointers)."""
    from chroma_amd import _lib
    threshold, W, H, pre, post = trig
    v = dict(nrows=ps.nrows, nchannels=ps.nchannels, window=_lib.DaqWindow(-8.0, 0.5, ps.nbins), trigger=_lib.DaqTrigger(0, threshold, W, H, pre, post),
             digitizer=dig_struct, seed=seed, acquisition=acquisition, offsets=ps.offsets, channel=ps.channel, bin=ps.bin, q_int=ps.q_int, npulses=len(ps),
             trig_offsets=np.ascontiguousarray(want['trig_offsets'], dtype=np.uint32), trig_bin=np.ascontiguousarray(want['trig_bin'], dtype=np.uint32),
             ntriggers=len(want['trig_bin']), hit_offsets=np.ascontiguousarray(want['hit_offsets'], dtype=np.uint32),
             hit_channel=np.ascontiguousarray(want['hit_channel'], dtype=np.int32), nhits=len(want['hit_channel']), first_hit=first_hit,
             nhits_call=nhits_call, capacity=capacity, adc=adc, flags=flags)
    v.update(change or {})
    return v


ORDER = ('nrows', 'nchannels', 'window', 'trigger', 'digitizer', 'seed', 'acquisition', 'offsets', 'channel', 'bin', 'q_int', 'npulses', 'trig_offsets',
         'trig_bin', 'ntriggers', 'hit_offsets', 'hit_channel', 'nhits', 'first_hit', 'nhits_call', 'capacity', 'adc', 'flags')
SENTINEL16, SENTINEL32 = 0xa5c3, 0xa5c3a5c3


def host_rc(ps, trig, want, dig, seed=SEED, acquisition=ACQUISITION, first_hit=0, nhits_call=None, capacity=None, guard=8, change=None, struct_change=None):
    """chroma_daq_digitize_host into sentinel-filled arrays `guard` entries longer than the slice needs; (rc, adc, flags)."""
    from chroma_amd import _lib
    G = trig[3] + trig[4]
    nhits = len(want['hit_channel'])
    nhits_call = nhits - first_hit if nhits_call is None else nhits_call
    room = max(0, min(nhits_call, nhits)) * min(G, 65536)
    adc = np.full(room + guard, SENTINEL16, dtype=np.uint16)
    flags = np.full(max(0, min(nhits_call, nhits)) + guard, SENTINEL32, dtype=np.uint32)
    v = call_arguments(ps, trig, want, dig.struct(**(struct_change or {})), seed, acquisition, first_hit, nhits_call, room if capacity is None else capacity,
                       adc, flags, change)
    args = [v[k] for k in ORDER]
    args = [_lib.ptr(a) if isinstance(a, np.ndarray) else ctypes.byref(a) if isinstance(a, ctypes.Structure) else a for a in args]
    return _lib.load().chroma_daq_digitize_host(*args), adc, flags


def assert_traces(adc, flags, want_adc, want_flags, what, guard=8):
    n, G = want_adc.shape
    assert len(adc) == n * G + guard and len(flags) == n + guard, what
    got = adc[:n * G].reshape(n, G)
    assert np.array_equal(got, want_adc), '%s: samples differ in traces %s' % (what, np.flatnonzero((got != want_adc).any(axis=1))[:8])
    assert np.array_equal(flags[:n], want_flags), '%s: flags\n%s\n%s' % (what, flags[:n], want_flags)
    assert (adc[n * G:] == SENTINEL16).all() and (flags[n:] == SENTINEL32).all(), '%s: words behind' % what


# ---- 1. the twin and the package are the restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', range(5))
def test_the_host_twin_and_digitize_are_the_restatement_on_the_trigger_sets(which):
    from chroma_amd.gpu.daq import DaqTrigger, EventTriggers
    dig = digitisers()[which]
    seen = dict.fromkeys(['inside', 'top', 'zero', 'before the window', 'beyond the window'], 0)
    gates = set()
    for index, (name, ps, trig) in enumerate(cases()):
        want = brute(index, 'nhit')
        want_adc, want_flags = brute_traces(index, which)
        what = '%s, %s' % (name, dig.name)
        rc, adc, flags = host_rc(ps, trig, want, dig)
        assert rc == 0, what
        assert_traces(adc, flags, want_adc, want_flags, what)
        got = ps.event_pulses().trigger(DaqTrigger(*trig)).digitize(dig.of_the_package(), seed=SEED, acquisition=ACQUISITION)
        assert isinstance(got, EventTriggers) and got.adc.dtype == np.uint16 and got.trace_flags.dtype == np.uint32
        assert got.adc.shape == want_adc.shape and np.array_equal(got.adc, want_adc) and np.array_equal(got.trace_flags, want_flags), what
        top = (1 << dig.bits) - 1
        seen['inside'] += int(((want_adc > 0) & (want_adc < top) & (want_adc != dig.pedestal)).sum())
        seen['top'] += int((want_flags & 1).sum())
        seen['zero'] += int((want_flags & 2).sum())
        b = want['trig_bin'].astype(np.int64)
        seen['before the window'] += int(((b - trig[3] < 0) & (np.diff(want['hit_offsets'].astype(np.int64)) > 0)).sum())
        seen['beyond the window'] += int(((b + trig[4] > ps.nbins) & (np.diff(want['hit_offsets'].astype(np.int64)) > 0)).sum())
        gates.add(trig[3] + trig[4])
    print(dig.name, seen)
    assert gates == {1, 4, 6, 7, 8, 16, 64, 100, 200}
    assert seen['top'] and seen['before the window'] and seen['beyond the window'], seen
    assert seen['inside'] or dig.bits == 1, seen
    assert seen['zero'] or (dig.taps >= 0).all(), seen


def test_the_host_twin_and_digitize_are_the_restatement_on_the_handmade_sets():
    from chroma_amd.gpu.daq import DaqTrigger
    for (name, ps, trig, dig), (want, want_adc, want_flags) in zip(handmade(), handmade_results()):
        assert len(want['hit_channel']) >= 1, name
        rc, adc, flags = host_rc(ps, trig, want, dig)
        assert rc == 0, name
        assert_traces(adc, flags, want_adc, want_flags, name)
        got = ps.event_pulses().trigger(DaqTrigger(*trig)).digitize(dig.of_the_package(), seed=SEED, acquisition=ACQUISITION)
        assert np.array_equal(got.adc, want_adc) and np.array_equal(got.trace_flags, want_flags), name


# ---- 2. the hand-made sets say what they were made to say ---------------------------------------------------------------------------------------
def made(name):
    """(PulseSet, trigger, Digitiser, the restated triggers, adc, trace_flags) of a hand-made set -- adc and trace_flags as the HOST
    TWIN gives them, which are the restatement's: the numbers the tests below derive by hand bind both."""
    index = [c[0] for c in handmade()].index(name)
    ps, trig, dig = handmade()[index][1:]
    want, want_adc, want_flags = handmade_results()[index]
    rc, adc, flags = host_rc(ps, trig, want, dig)
    assert rc == 0
    assert_traces(adc, flags, want_adc, want_flags, name)
    n = len(want_adc)
    return ps, trig, dig, want, adc[:want_adc.size].reshape(want_adc.shape), flags[:n]


def test_a_pulse_counts_up_to_ntaps_minus_one_bins_before_the_first_sample():
    ps, trig, dig, want, adc, flags = made('reach of the taps')
    assert want['trig_bin'].tolist() == [20] and want['hit_channel'].tolist() == [0, 1]
    # sample 0 is bin 18: channel 0 has its pulse of bin 14 on tap 4 (1000 * 16 >> 8 = 62), channel 1 has nothing of bin 13
    assert adc[0, 0] == 7 + 62 and adc[1, 0] == 7 and adc[0, 1] == 7 and adc[:, 2].tolist() == [7 + 3, 7 + 3] and not flags.any()


def test_the_tail_of_a_pulse_in_the_gate_before_is_on_the_line():
    ps, trig, dig, want, adc, flags = made('tail from the gate before')
    assert want['trig_bin'].tolist() == [20, 26] and want['pulse_trigger'].tolist() == [0, 0, 1, 1]
    # the second trace begins at bin 24: 5000 on tap 2 and 100 on tap 4, then the pulses of bins 26 and 27 on top
    assert adc[1].tolist() == [(100 * 16 + 5000 * 64) >> 8, (100 * 8 + 5000 * 32) >> 8, (100 * 4 + 5000 * 16 + 10 * 256) >> 8,
                               (100 * 2 + 5000 * 8 + 10 * 128 + 20 * 256) >> 8, (5000 * 4 + 10 * 64 + 20 * 128) >> 8, (5000 * 2 + 10 * 32 + 20 * 64) >> 8]
    # without the pulse of bin 22 the second trace is another
    assert adc[1, 0] != (100 * 16) >> 8


def test_more_than_a_wave_of_pulses_reaches_one_sample_and_the_trace_runs_beyond_the_window():
    ps, trig, dig, want, adc, flags = made('150 pulses under 100 taps')
    assert want['trig_bin'].tolist() == [10] and adc.shape == (1, 200) and ps.nbins == 200
    taps, q = dig.taps.astype(np.int64), ps.q_int.astype(np.int64)
    for s in (99, 120, 149, 190, 199):          # (bins 109 .. 209: 100, 100, 100, 59 and 50 pulses in reach)
        acc = sum(int(q[p]) * int(taps[10 + s - (10 + p)]) for p in range(150) if 0 <= s - p < 100)
        assert adc[0, s] == min(max(50 + (acc >> 10), 0), 65535) and 50 < adc[0, s] < 65535


def test_saturation_sets_exactly_the_flags_expected():
    ps, trig, dig, want, adc, flags = made('saturation')
    assert want['trig_bin'].tolist() == [10] and want['hit_channel'].tolist() == [0, 1, 2, 3, 4]
    assert flags.tolist() == [0, 1, 2, 0, 3]
    assert adc[1].tolist() == [100] * 7 + [4095] and adc[2].tolist() == [0] + [100] * 7 and adc[4].tolist() == [100] * 3 + [4095, 0] + [100] * 3
    assert (adc[0] == 100).all() and (adc[3] == 100).all()


def test_the_sum_wraps_in_64_bits():
    ps, trig, dig, want, adc, flags = made('the sum wraps')
    assert want['trig_bin'].tolist() == [10]
    # gate [8, 16).  One pulse in reach: -(2^32 - 1) 2^31, clipped at 0.  Two: -2^64 + 2^32 wraps to 2^32, clipped at the top.
    # Three: -3 2^63 + 3 2^31 wraps to -2^63 + 3 2^31, clipped at 0.
    assert adc[0].tolist() == [0, 0, 0, 65535, 0, 65535, 0, 0] and flags.tolist() == [3]


def test_a_trigger_without_hits_has_no_trace_and_a_row_without_pulses_none():
    ps, trig, dig, want, adc, flags = made('a trigger without hits')
    assert want['trig_offsets'].tolist() == [0, 4, 4, 8] and np.diff(want['hit_offsets'].astype(np.int64)).tolist() == [1, 0, 0, 0, 2, 0, 0, 0]
    assert adc.shape == (3, 1)


# ---- 3. properties ---------------------------------------------------------------------------------------------------------------------------
def test_unit_taps_give_the_clipped_charge_counts_of_the_waveform():
    from chroma_amd.gpu.daq import DaqTrigger, DaqDigitizer
    index = 1
    name, ps, trig = cases()[index]
    small = PulseSet(ps.nrows, ps.nchannels, ps.nbins, ps.offsets, ps.channel, ps.bin, ps.npe, ps.q_int % 70000, ps.t_first, ps.flags)
    pulses = small.event_pulses()
    shift = 16
    got = pulses.trigger(DaqTrigger(*trig)).digitize(DaqDigitizer([1.0 / CHARGE_UNIT], pedestal=0, bits=16, shift=shift))
    assert got.digitizer.tables(CHARGE_UNIT)[0].tolist() == [1 << shift]
    pre, G = trig[3], trig[3] + trig[4]
    ntested = nclipped = 0
    for r in range(ps.nrows):
        t = got.event(r)
        for k in range(len(t)):
            channels, traces = t.adc(k)
            assert traces.shape == (len(channels), G) and np.array_equal(channels, t.sparse(k)[0])
            for c, trace in zip(channels, traces):
                npe, q = pulses.event(r).waveform(c)
                counts = (q.astype(np.float64) / CHARGE_UNIT).astype(np.int64)          # (below 2^24: exact)
                bins = int(t.bin[k]) - pre + np.arange(G)
                inside = (bins >= 0) & (bins < ps.nbins)
                want = np.zeros(G, dtype=np.int64)
                want[inside] = np.minimum(counts[bins[inside]], 65535)
                assert np.array_equal(trace, want) and np.array_equal(t.trace(k, c), trace)
                ntested += 1
                nclipped += int((want == 65535).any())
            assert np.array_equal(t.sample_times(k), -8.0 + 0.5 * (int(t.bin[k]) - pre + np.arange(G, dtype=np.float64)))
    assert ntested > 20 and nclipped >= 1


def rows_of(ps, want, rows):
    """The PulseSet and the trigger arrays of the rows [rows[0], rows[1]) alone, and the slice of their hits."""
    a, b = rows
    p0, p1 = int(ps.offsets[a]), int(ps.offsets[b])
    t0, t1 = int(want['trig_offsets'][a]), int(want['trig_offsets'][b])
    h0, h1 = int(want['hit_offsets'][t0]), int(want['hit_offsets'][t1])
    sub = PulseSet(b - a, ps.nchannels, ps.nbins, ps.offsets[a:b + 1] - ps.offsets[a], ps.channel[p0:p1], ps.bin[p0:p1], ps.npe[p0:p1], ps.q_int[p0:p1],
                   ps.t_first[p0:p1], ps.flags[p0:p1])
    sub_want = dict(trig_offsets=want['trig_offsets'][a:b + 1] - np.uint32(t0), trig_bin=want['trig_bin'][t0:t1],
                    hit_offsets=want['hit_offsets'][t0:t1 + 1] - np.uint32(h0), hit_channel=want['hit_channel'][h0:h1])
    return sub, sub_want, slice(h0, h1)


def test_row_r_of_a_call_is_row_0_of_a_call_with_acquisition_plus_r():
    index, which = 1, 1          # (a digitiser with noise)
    name, ps, trig = cases()[index]
    want = brute(index, 'nhit')
    want_adc, want_flags = brute_traces(index, which)
    ncompared = 0
    for r in range(ps.nrows):
        sub, sub_want, hits = rows_of(ps, want, (r, r + 1))
        rc, adc, flags = host_rc(sub, trig, sub_want, digitisers()[which], acquisition=(ACQUISITION + r) & 0xffffffff)
        assert rc == 0
        assert_traces(adc, flags, want_adc[hits], want_flags[hits], 'row %d alone' % r)
        ncompared += hits.stop - hits.start
    assert ncompared == len(want_adc) > 20


def test_the_noise_of_a_bin_is_the_same_whichever_firing_reads_it():
    """Taps of 0: a trace is pedestal plus noise.  The same pulses under two gates that begin 3 bins apart: where the gates read the
    same (row, channel, bin) they read the same sample."""
    index = 0
    name, ps, (threshold, W, H, pre, post) = cases()[index]
    dig = Digitiser('noise alone', [0], 0, 1000, 12, 5.0)
    results = {}
    for shift_by in (0, 3):
        trig = (threshold, W, H + 3, pre + shift_by, post)
        want = brute_of(ps, 'nhit', *trig)
        rc, adc, flags = host_rc(ps, trig, want, dig)
        assert rc == 0
        n = len(want['hit_channel'])
        adc = adc[:n * (pre + shift_by + post)].reshape(n, -1)
        assert np.array_equal(adc, brute_adc(ps, trig, want, dig)[0])
        of = np.repeat(np.arange(len(want['trig_bin'])), np.diff(want['hit_offsets'].astype(np.int64)))
        results[shift_by] = {(int(k), int(c)): trace for k, c, trace in zip(of, want['hit_channel'], adc)}, want['trig_bin']
    assert np.array_equal(results[0][1], results[3][1])          # (the gate does not move the firings)
    common = sorted(set(results[0][0]) & set(results[3][0]))
    assert len(common) > 10
    for key in common:
        assert np.array_equal(results[0][0][key], results[3][0][key][3:]), key
    values = np.concatenate([results[0][0][key] for key in common]).astype(np.int64) - 1000
    assert len(set(values.tolist())) > 10 and abs(values.mean()) < 2.0


def test_a_slice_is_that_part_of_the_whole():
    index, which = 1, 4
    name, ps, trig = cases()[index]
    want = brute(index, 'nhit')
    want_adc, want_flags = brute_traces(index, which)
    nhits = len(want_adc)
    inside = int(want['hit_offsets'][1]) + 1          # (inside the hits of the second trigger)
    assert want['hit_offsets'][1] < inside < want['hit_offsets'][2]
    for first, n in ((0, 1), (inside, 7), (nhits - 1, 1), (3, nhits - 3), (5, 0), (nhits, 0)):
        rc, adc, flags = host_rc(ps, trig, want, digitisers()[which], first_hit=first, nhits_call=n)
        assert rc == 0
        assert_traces(adc, flags, want_adc[first:first + n], want_flags[first:first + n], 'hits [%d, %d)' % (first, first + n))


@functools.lru_cache(maxsize=None)
def noise_words():
    """The words of bins 0 .. 2^16 - 1 of channel 3 in stream 5."""
    blocks = {}
    return np.array([philox_word(blocks, SEED, 5, 3, 65536 + b) for b in range(1 << 16)], dtype=np.uint32)


def test_the_noise_table_of_the_package():
    from chroma_amd.gpu.daq import DaqDigitizer
    for sigma in (0.3, 1.0, 2.5, 8.0):
        taps, cdf, lo = DaqDigitizer([1.0], noise_sigma=sigma).tables(1.0)
        assert lo == NOISE_LO and cdf.dtype == np.uint32 and len(cdf) == 64 and np.array_equal(cdf, noise_table(sigma))
        assert (np.diff(cdf.astype(np.int64)) >= 0).all()
        # over 2^16 consecutive bins of one channel: the mean within 0.1 count, the variance within 5 % of sigma^2 + 1/12 (a
        # Gaussian rounded to whole counts; the table's +- 32 counts are 4 sigma at the least)
        values = (NOISE_LO + np.searchsorted(cdf, noise_words(), side='right')).astype(np.float64)          # (#{j : w >= cdf[j]})
        print('sigma %g: mean %.4f, variance %.4f (%.4f)' % (sigma, values.mean(), values.var(), sigma ** 2 + 1.0 / 12.0))
        # what the table itself says: value noise_lo + k has the probability (cdf[k] - cdf[k - 1]) / 2^32 (cdf[-1] = 0, cdf[64] = 2^32)
        p = np.diff(np.concatenate(([0.0], cdf.astype(np.float64), [2.0 ** 32]))) / 2.0 ** 32
        k = NOISE_LO + np.arange(65, dtype=np.float64)
        exact_mean = float((p * k).sum())
        exact_var = float((p * (k - exact_mean) ** 2).sum())
        print('    the table: mean %.6f, variance %.6f' % (exact_mean, exact_var))
        assert abs(exact_mean) < 1e-6 and abs(values.mean()) < 0.1
        # the samples against the table at every sigma (the relative spread of a sample variance over 2^16 draws is 1.2 % at sigma 0.3,
        # where the values are -1, 0 and 1, and 0.6 % for a Gaussian) ...
        assert abs(values.var() / exact_var - 1.0) < 0.05
        # ... and the table against the Gaussian: rounding to whole counts adds 1/12 where sigma is no smaller than a count; below, the
        # variance is that of the three values -1, 0, 1: 2 (1 - Phi(0.5 / sigma)) up to the tails beyond 1.5 counts
        if sigma >= 1.0:
            assert abs(values.var() / (sigma ** 2 + 1.0 / 12.0) - 1.0) < 0.05 and abs(exact_var / (sigma ** 2 + 1.0 / 12.0) - 1.0) < 0.01
        else:
            import math
            tails = lambda x: 1.0 - math.erf(x / sigma / math.sqrt(2.0))          # (2 (1 - Phi(x / sigma)))
            assert abs(exact_var - (tails(0.5) + 3.0 * tails(1.5))) < 1e-6          # (1 on +-1, 4 on +-2: nothing beyond at sigma 0.3)
    assert DaqDigitizer([1.0], noise_sigma=0.3).tables(1.0)[1][-1] == 0xffffffff          # (saturated: Phi is 1 in float64 there)
    assert len(DaqDigitizer([1.0]).tables(1.0)[1]) == 0
    with pytest.raises(ValueError):
        DaqDigitizer([1.0], noise_sigma=8.01)
    with pytest.raises(ValueError):
        DaqDigitizer([1.0], noise_sigma=-1.0)


def test_daq_digitizer_validates_and_makes_its_taps():
    from chroma_amd.gpu.daq import DaqDigitizer, DaqTrigger
    d = DaqDigitizer([0.5, -0.25, 0.1], pedestal=20, bits=12, shift=10)
    taps, cdf, lo = d.tables(0.125)
    assert taps.dtype == np.int32 and taps.tolist() == [64, -32, 13]          # round(shape * 0.125 * 1024)
    assert d == DaqDigitizer([0.5, -0.25, 0.1], pedestal=20, bits=12, shift=10) and hash(d) == hash(DaqDigitizer([0.5, -0.25, 0.1], 20, 12, 10))
    assert d != DaqDigitizer([0.5, -0.25, 0.1], pedestal=21, bits=12, shift=10) and DaqDigitizer.of(d) is d and 'bits=12' in repr(d)
    struct, keep = d.struct(0.125)
    assert (struct.ntaps, struct.shift, struct.pedestal, struct.bits, struct.nnoise, struct.noise_lo) == (3, 10, 20, 12, 0, NOISE_LO)
    assert ctypes.sizeof(struct) == 40
    b = DaqDigitizer.biexponential(10.0, 2.0, 10.0, 0.5)
    assert (b.bits, b.pedestal, b.shift, b.noise_sigma) == (14, 0, 16, 0.0) and 1 < len(b.shape) <= 1024
    assert 9.5 < b.shape.max() <= 10.0 and b.shape[0] > 0 and b.shape[-1] < 0.02 and np.argmax(b.shape) in (7, 8)          # (the curve peaks at 4.02 ns)
    assert len(DaqDigitizer.biexponential(10.0, 2.0, 10.0, 0.5, length=40).shape) == 40 and len(DaqDigitizer.biexponential(1.0, 2.0, 500.0, 0.5).shape) == 1024
    assert DaqDigitizer.of((10.0, 2.0, 10.0, 0.5, 12, 100, 1.5)) == DaqDigitizer.biexponential(10.0, 2.0, 10.0, 0.5, bits=12, pedestal=100, noise_sigma=1.5)
    for bad in (dict(shape=[]), dict(shape=[1.0] * 1025), dict(shape=[float('nan')]), dict(shape=[[1.0]]), dict(shape=[1.0], bits=0), dict(shape=[1.0], bits=17),
                dict(shape=[1.0], shift=32), dict(shape=[1.0], shift=-1), dict(shape=[1.0], pedestal=1 << 31), dict(shape=[1.0], bits=2.5)):
        with pytest.raises(ValueError):
            DaqDigitizer(**bad)
    for bad in ((10.0, 10.0, 2.0, 0.5), (10.0, 0.0, 2.0, 0.5), (10.0, 2.0, 10.0, 0.0), (10.0, 2.0, 10.0, 0.5, 2000)):
        with pytest.raises(ValueError):
            DaqDigitizer.biexponential(*bad)
    for bad in (3, (1.0, 2.0, 3.0), 'abcd', (1, 2, 3, 4, 5, 6, 7, 8)):
        with pytest.raises(ValueError):
            DaqDigitizer.of(bad)
    with pytest.raises(ValueError):
        DaqDigitizer([1e6]).tables(1.0)          # (1e6 * 2^16 does not fit 32 bits)
    with pytest.raises(ValueError):
        DaqDigitizer([1.0]).check(DaqTrigger(1, 1, 70000, 30000, 35537))
    assert DaqDigitizer([1.0]).check(DaqTrigger(1, 1, 70000, 30000, 35536)).bits == 14
    # triggers that were not digitised say so
    t = cases()[0][1].event_pulses().trigger(DaqTrigger(*cases()[0][2]))
    assert t.adc is None and t.trace_flags is None and t.digitizer is None
    with pytest.raises(ValueError):
        t.event(0).adc(0)
    digitised = t.digitize(d)
    nabsent = 0
    for r in np.flatnonzero(np.diff(digitised.offsets)):
        ev = digitised.event(r)
        for absent in set(range(5)) - set(ev.adc(0)[0].tolist()):
            with pytest.raises(KeyError):
                ev.trace(0, absent)
            nabsent += 1
        with pytest.raises(IndexError):
            ev.trace(0, 5)
        with pytest.raises(IndexError):
            ev.sample_times(len(ev))
    assert nabsent >= 1


def noise_only(dig, trig, stream_row, channel, b):
    """The trace of a hit without signal: pedestal plus the noise of (row, channel word, bin), clipped."""
    blocks = {}
    out = []
    for s in range(trig[3] + trig[4]):
        w = philox_word(blocks, SEED, (1 + ACQUISITION + stream_row) & 0xffffffff, channel & 0xffffffff, b - trig[3] + s + 65536)
        out.append(min(max(dig.pedestal + NOISE_LO + int((w >= dig.noise_cdf.astype(np.int64)).sum()), 0), (1 << dig.bits) - 1))
    return out


def garbage_case():
    """cases()[0] with hits whose channel is nchannels or -1, and trigger offsets that begin at 1 so that trigger 0 lies in no row:
    (PulseSet, trigger, Digitiser, the changed trigger arrays, adc, trace_flags).  The traces of those hits are pedestal plus noise (of
    row 0 where there is no row, of the channel word as it stands), every other trace is what it was."""
    index, which = 0, 1
    name, ps, trig = cases()[index]
    dig = digitisers()[which]
    want = dict(brute(index, 'nhit'))
    want_adc, want_flags = [a.copy() for a in brute_traces(index, which)]
    assert int(want['trig_offsets'][1]) >= 1 and int(want['hit_offsets'][1]) >= 1          # (trigger 0 is of row 0 and has hits)
    rows = np.repeat(np.arange(ps.nrows), np.diff(want['trig_offsets'].astype(np.int64)))
    of = np.repeat(np.arange(len(want['trig_bin'])), np.diff(want['hit_offsets'].astype(np.int64)))
    channel = want['hit_channel'].copy()
    outside = {len(channel) - 1: ps.nchannels, len(channel) - 3: -1}
    trig_offsets = want['trig_offsets'].copy()
    trig_offsets[0] = 1
    nchanged = 0
    for i in range(len(channel)):
        c = outside.get(i, int(channel[i]))
        if i in outside or of[i] == 0:
            channel[i] = c
            want_adc[i] = noise_only(dig, trig, 0 if of[i] == 0 else int(rows[of[i]]), c, int(want['trig_bin'][of[i]]))
            want_flags[i] = 0          # (a pedestal of 2000 in 12 bits, noise of +- 32: never clipped)
            assert 0 < want_adc[i].min() and want_adc[i].max() < (1 << dig.bits) - 1
            nchanged += 1
    assert 3 <= nchanged < len(channel) - 5
    return ps, trig, dig, dict(want, hit_channel=channel, trig_offsets=trig_offsets), want_adc, want_flags


def test_a_channel_outside_the_detector_and_a_trigger_in_no_row_have_no_signal():
    ps, trig, dig, want, want_adc, want_flags = garbage_case()
    rc, adc, flags = host_rc(ps, trig, want, dig)
    assert rc == 0
    assert_traces(adc, flags, want_adc, want_flags, 'entries that count for nothing')
    assert not np.array_equal(want_adc, brute_traces(0, 1)[0])


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------------------------
def refusals():
    """[(what, keyword arguments of host_rc / device_rc that make the call one to refuse)] on cases()[0]: 70 bins; threshold 3, W 4, H 6, pre 2, post 4."""
    name, ps, trig = cases()[0]
    nhits = len(brute(0, 'nhit')['hit_channel'])
    decreasing = np.array([5, 9, 8, 20], dtype=np.uint32)
    from chroma_amd import _lib
    T = lambda *t: dict(change=dict(trigger=_lib.DaqTrigger(*t)))
    W = lambda *w: dict(change=dict(window=_lib.DaqWindow(*w)))
    return [('threshold 0', T(0, 0, 4, 6, 2, 4)), ('width 0', T(0, 3, 0, 6, 2, 4)), ('width beyond the window', T(0, 3, 71, 80, 2, 4)), ('post 0', T(0, 3, 4, 6, 2, 0)),
            ('holdoff below pre + post', T(0, 3, 4, 5, 2, 4)), ('pre + post beyond 32 bits', T(0, 3, 4, 6, 0xffffffff, 8)), ('an unknown kind', T(2, 3, 4, 6, 2, 4)),
            ('a gate of 65537 samples', T(0, 3, 4, 70000, 65533, 4)), ('no bins', W(-8.0, 0.5, 0)), ('65537 bins', W(-8.0, 0.5, 65537)), ('dt 0', W(-8.0, 0.0, 70)),
            ('dt NaN', W(-8.0, float('nan'), 70)), ('t0 infinite', W(float('inf'), 0.5, 70)), ('no rows', dict(change=dict(nrows=0))),
            ('no channels', dict(change=dict(nchannels=0))), ('2^31 channels', dict(change=dict(nchannels=1 << 31))),
            ('rows * bins of 2^31', dict(change=dict(nrows=(1 << 31) // 70 + 1))), ('no taps', dict(struct_change=dict(ntaps=0))),
            ('1025 taps', dict(struct_change=dict(ntaps=1025))), ('a NULL tap table', dict(struct_change=dict(taps=None))), ('a shift of 32', dict(struct_change=dict(shift=32))),
            ('no bits', dict(struct_change=dict(bits=0))), ('17 bits', dict(struct_change=dict(bits=17))), ('65 noise entries', dict(struct_change=dict(nnoise=65))),
            ('a NULL noise table', dict(struct_change=dict(noise_cdf=None, nnoise=4))),
            ('a descending noise table', dict(struct_change=dict(noise_cdf=_lib.ptr(decreasing), nnoise=4), keep=decreasing)),
            ('2^32 pulses', dict(change=dict(npulses=1 << 32))), ('2^32 hits', dict(change=dict(nhits=1 << 32))), ('2^32 triggers', dict(change=dict(ntriggers=1 << 32))),
            ('no pulse channels', dict(change=dict(channel=None))), ('no offsets', dict(change=dict(offsets=None))),
            ('no pulse bins', dict(change=dict(bin=None))), ('no charge counts', dict(change=dict(q_int=None))), ('no trigger offsets', dict(change=dict(trig_offsets=None))),
            ('no trigger bins', dict(change=dict(trig_bin=None))), ('no hit offsets', dict(change=dict(hit_offsets=None))), ('no hit channels', dict(change=dict(hit_channel=None))),
            ('no samples', dict(change=dict(adc=None))), ('no flag words', dict(change=dict(flags=None))), ('no window', dict(change=dict(window=None))),
            ('no trigger', dict(change=dict(trigger=None))), ('no digitiser', dict(change=dict(digitizer=None))),
            ('a slice that begins beyond the hits', dict(first_hit=nhits + 1, nhits_call=0)), ('a slice that ends beyond the hits', dict(first_hit=nhits - 2, nhits_call=3)),
            ('a slice of 2^64 - 1 hits', dict(first_hit=1, nhits_call=(1 << 64) - 1)), ('room for one sample too few', dict(capacity=nhits * 6 - 1))]


def test_the_host_twin_refuses_what_the_header_says_and_writes_nothing():
    name, ps, trig = cases()[0]
    want = brute(0, 'nhit')
    assert len(want['hit_channel']) > 3
    for what, kw in refusals():
        kw = dict(kw)
        kw.pop('keep', None)
        given = (kw.get('change') or {})
        rc, adc, flags = host_rc(ps, trig, want, digitisers()[1], **kw)
        assert rc == ERR_INVALID, what
        if 'adc' not in given and 'flags' not in given:
            assert (adc == SENTINEL16).all() and (flags == SENTINEL32).all(), what
    from chroma_amd import _lib
    assert b'room for fewer samples' in _lib.load().chroma_last_error()
    rc, adc, flags = host_rc(ps, trig, want, digitisers()[1], first_hit=2, nhits_call=0, change=dict(adc=None, flags=None))
    assert rc == 0          # (no hits in the call: no arrays needed)


def test_digitize_and_acquire_pulses_refuse_what_does_not_fit():
    from chroma_amd.gpu.daq import DaqTrigger, DaqDigitizer, EventTriggers, GPUEventDaq
    name, ps, trig = cases()[0]
    t = ps.event_pulses().trigger(DaqTrigger(*trig))
    with pytest.raises(ValueError):
        t.digitize(DaqDigitizer([1e7]))          # (the taps do not fit)
    bare = EventTriggers(t.window, t.trigger, t.nchannels, t.charge_unit, t.pulse_offsets, t.offsets, t.bin, t.sum, t.hit_offsets, t.hit_channel, t.hit_npe,
                         t.hit_q_int, t.hit_t_first, t.hit_flags, t.pulse_trigger)
    with pytest.raises(ValueError, match='do not hold their pulses'):
        bare.digitize(DaqDigitizer([1.0]))
    daq = object.__new__(GPUEventDaq)          # (no context: anything but the refusal would fail on a missing attribute)
    with pytest.raises(ValueError, match='digitizer needs trigger'):
        daq.acquire_pulses(None, None, [0, 1], (-8.0, 0.5, 70), digitizer=DaqDigitizer([1.0]))


def test_simulate_refuses_a_digitiser_without_a_trigger_before_it_touches_a_gpu():
    from chroma_amd import event
    from chroma_amd.gpu.daq import DaqDigitizer
    from chroma_amd.sim import Simulation
    sim = object.__new__(Simulation)          # (no context, no geometry: anything but the refusal would fail on a missing attribute)
    with pytest.raises(ValueError, match='daq_digitizer needs daq_trigger'):
        next(sim.simulate([event.Photons()], run_daq=True, daq_window=(-8.0, 0.5, 64), daq_digitizer=DaqDigitizer([1.0])))
    with pytest.raises(ValueError, match='daq_trigger needs daq_window'):
        next(sim.simulate([event.Photons()], run_daq=True, daq_trigger=(3, 4), daq_digitizer=DaqDigitizer([1.0])))


def test_chroma_sim_refuses_a_bad_digitiser_before_it_touches_a_gpu(capsys):
    from chroma_amd import cli
    window_and_trigger = ['--daq-window=-8,0.5,512', '--daq-trigger', '2,16,64,8,40']
    for argv, message in ((['--daq-digitize', '10,2,10'], '--daq-digitize needs --daq-trigger'),
                          (['--daq-window=-8,0.5,512', '--daq-digitize', '10,2,10'], '--daq-digitize needs --daq-trigger'),
                          (window_and_trigger + ['--daq-digitize', '10,2'], '--daq-digitize takes AMPLITUDE,RISE_NS,FALL_NS'),
                          (window_and_trigger + ['--daq-digitize', '10,2,10,14,0,1,7'], '--daq-digitize takes AMPLITUDE,RISE_NS,FALL_NS'),
                          (window_and_trigger + ['--daq-digitize', '10,12,10'], '--daq-digitize: a biexponential pulse needs'),
                          (window_and_trigger + ['--daq-digitize', '10,2,10,17'], '--daq-digitize: a digitiser\'s bits'),
                          (window_and_trigger + ['--daq-digitize', '10,2,10,14,0,9'], '--daq-digitize: a digitiser\'s noise'),
                          (window_and_trigger + ['--daq-digitize', '10,2,x'], '--daq-digitize: could not convert')):
        with pytest.raises(SystemExit):
            cli.main(['@chroma_amd.demo.tiny'] + argv)
        assert message in capsys.readouterr().err, argv
