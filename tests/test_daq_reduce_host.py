"""The trace reduction of the time-binned DAQ on the host (no GPU): chroma_daq_reduce_host and EventTriggers.reduce, bit for bit on
a brute-force restatement of the definition in include/chroma_hip.h ("trace reduction") in Python integers -- on the traces of the
digitiser tests' restatement, on hand-made traces at the edges of the definition and on random ones -- and what follows from the
definitions exactly: the integral of a lone pulse is the sum of its samples' signal, and moving it by k bins moves its time by
256 k.  tests/test_gpu_daq_reduce.py holds the device call to the same restatement on the same sets.
"""
import ctypes
import functools

import numpy as np
import pytest

from test_daq_trigger_host import cases, from_rows
from test_daq_digitize_host import digitisers, brute_traces, CHARGE_UNIT

ERR_INVALID = -1
SENTINEL32, SENTINEL64, SENTINEL_N = 0xdeadbeef, 0x5a5a5a5a5a5a5a5a, 0xfeedfacefeedface
TIME_AT_EDGE, OPEN_AT_START, OPEN_AT_END, BASELINE_BUSY = 1, 2, 4, 1
FIELDS = ('polarity', 'nbaseline', 'pedestal', 'baseline_spread', 'threshold', 'min_width', 'lead', 'lag', 'cfd')
PER_TRACE = (('found_offsets', np.uint32), ('trace_base', np.int32), ('reduced_flags', np.uint32))
PER_PULSE = (('found_start', np.uint32), ('found_width', np.uint32), ('found_peak', np.uint32), ('found_peak_sample', np.uint32),
             ('found_integral', np.int64), ('found_time', np.uint32), ('found_flags', np.uint32))


class Reducer(object):
    """A chroma_daq_reducer as integers (cfd in 1/256).  nbaseline 'G': the whole trace, for traces of 64 samples at the most."""

    def __init__(self, name, threshold, polarity=1, nbaseline=0, pedestal=0, baseline_spread=0, min_width=1, lead=0, lag=0, cfd=128):
        self.name = name
        self.threshold, self.polarity, self.nbaseline, self.pedestal, self.baseline_spread = threshold, polarity, nbaseline, pedestal, baseline_spread
        self.min_width, self.lead, self.lag, self.cfd = min_width, lead, lag, cfd

    def at(self, G):
        """This reducer on traces of G samples, or None where the contract refuses it (a baseline longer than the trace)."""
        nbaseline = G if self.nbaseline == 'G' else self.nbaseline
        if nbaseline > G or nbaseline > 64:
            return None
        return Reducer(self.name, self.threshold, self.polarity, nbaseline, self.pedestal, self.baseline_spread, self.min_width, self.lead, self.lag, self.cfd)

    def struct(self, **change):
        from chroma_amd import _lib
        v = {k: getattr(self, k) for k in FIELDS}
        v.update(change)
        return _lib.DaqReducer(*[v[k] for k in FIELDS])

    def of_the_package(self):
        from chroma_amd.gpu.daq import DaqReducer
        return DaqReducer(self.threshold, polarity=self.polarity, nbaseline=self.nbaseline, pedestal=self.pedestal, baseline_spread=self.baseline_spread,
                          min_width=self.min_width, lead=self.lead, lag=self.lag, cfd=self.cfd / 256.0)


@functools.lru_cache(maxsize=None)
def reducers():
    """Polarity -1; nbaseline 0, 1, 16, 64 and == G; min_width 2; lead and lag both 0 and both larger than every G of the sets;
    cfd 1, 128 and 256.  The pedestals are those of digitisers() (100, 2000, 30000, -3 -- clipped to 1 bit: 0 --, 300)."""
    return [Reducer('pedestal 100, lead = lag = 0', 3, pedestal=100),
            Reducer('falling, pedestal 2000', 2, polarity=-1, pedestal=2000, lead=2, lag=3, cfd=64),
            Reducer('pedestal 30000, min_width 2', 50, pedestal=30000, min_width=2, lead=1, lag=1, cfd=200),
            Reducer('pedestal 0, cfd 256', 1, lead=1, cfd=256),
            Reducer('pedestal 300, lead and lag beyond G', 2, pedestal=300, lead=300, lag=65535, cfd=1),
            Reducer('baseline of 1', 5, nbaseline=1, lead=1, lag=1, cfd=256),
            Reducer('baseline of 16', 2, nbaseline=16, baseline_spread=4, min_width=2, lead=3, lag=2, cfd=1),
            Reducer('baseline of 64', 1, nbaseline=64, baseline_spread=10, lead=65535, lag=65535),
            Reducer('falling, baseline of G', 1, polarity=-1, nbaseline='G', min_width=2, lead=2, cfd=200)]


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def brute_reduce(adc, r):
    """The definition, trace by trace in Python integers: a dict of found_offsets (traces + 1), trace_base, reduced_flags and the
    per-pulse arrays."""
    adc = np.asarray(adc)
    out = {name: [] for name, _ in PER_TRACE + PER_PULSE}
    out['found_offsets'].append(0)
    for trace in adc:
        v = [int(x) for x in trace]
        G = len(v)
        N = max(r.nbaseline, 1)
        base = sum(v[:r.nbaseline]) if r.nbaseline > 0 else r.pedestal
        y = [r.polarity * (N * x - base) for x in v]
        T = N * r.threshold
        busy = r.nbaseline > 0 and max(v[:r.nbaseline]) - min(v[:r.nbaseline]) > r.baseline_spread
        runs, s = [], 0
        while s < G:
            if y[s] >= T:
                a = s
                while s < G and y[s] >= T:
                    s += 1
                runs.append((a, s))
            else:
                s += 1
        pulses = [(a, e) for a, e in runs if e - a >= r.min_width]
        stops = []
        for j, (a, e) in enumerate(pulses):
            stop = min(e + r.lag, pulses[j + 1][0] if j + 1 < len(pulses) else G, G)
            begin = max(max(a - r.lead, 0), stops[j - 1] if j > 0 else 0)
            stops.append(stop)
            peak = max(y[a:e])
            peak_sample = a + y[a:e].index(peak)
            L = max(1, (peak * r.cfd) >> 8)
            s_c = peak_sample          # (y(peak_sample) = peak >= L)
            while s_c > begin and y[s_c - 1] >= L:
                s_c -= 1
            assert all(y[u] >= L for u in range(s_c, peak_sample + 1)) and (s_c == begin or y[s_c - 1] < L)
            flags = (OPEN_AT_START if a == 0 else 0) | (OPEN_AT_END if e == G else 0)
            if s_c == begin and (begin == 0 or y[begin - 1] >= L):
                time, flags = 256 * s_c, flags | TIME_AT_EDGE
            else:
                y0, y1 = y[s_c - 1], y[s_c]
                assert y0 < L <= y1 and 0 < (L - y0) * 256 < 1 << 31
                time = 256 * (s_c - 1) + ((L - y0) * 256) // (y1 - y0)
            for name, value in zip([n for n, _ in PER_PULSE], (a, e - a, peak, peak_sample, sum(y[begin:stop]), time, flags)):
                out[name].append(value)
        out['found_offsets'].append(len(out['found_start']))
        out['trace_base'].append(base)
        out['reduced_flags'].append(BASELINE_BUSY if busy else 0)
    return {name: np.array(out[name], dtype=kind) for name, kind in PER_TRACE + PER_PULSE}


@functools.lru_cache(maxsize=None)
def digitised_sets():
    """[(name, adc, Reducer, restatement)]: the traces of brute_traces(index, which) under every reducer that fits their length."""
    out = []
    for index, (name, ps, trig) in enumerate(cases()):
        for which, dig in enumerate(digitisers()):
            adc = brute_traces(index, which)[0]
            for r in reducers():
                r = r.at(adc.shape[1])
                if r is not None:
                    out.append(('%s, %s, %s' % (name, dig.name, r.name), adc, r, brute_reduce(adc, r)))
    return out


def trace(G, *runs, **kw):
    """One trace of G samples of `low` with the samples of every (a, e[, value]) run at `value` (default `high`)."""
    t = np.full(G, kw.get('low', 0), dtype=np.uint16)
    for run in runs:
        t[run[0]:run[1]] = run[2] if len(run) > 2 else kw.get('high', 50)
    return t


@functools.lru_cache(maxsize=None)
def handmade():
    """[(name, adc (traces x G), Reducer)]: the edges of the definition."""
    out = []
    plain = Reducer('threshold 10', 10, lead=2, lag=2)
    for G in (1, 2, 63, 64, 65, 128, 129, 200):
        out.append(('G = %d: nothing above, everything above, the ends' % G,
                    np.array([trace(G), trace(G, (0, G)), trace(G, (0, 1)), trace(G, (G - 1, G)), trace(G, (0, 1), (G - 1, G))]), plain))
    # the round boundary of the device walk
    out.append(('runs over samples 63 / 64', np.array([trace(129, (62, 66)), trace(129, (60, 64)), trace(129, (64, 70)), trace(129, (60, 64), (64, 70, 90))]), plain))
    alternating = trace(200, *[(s, s + 1) for s in range(0, 200, 2)])
    out.append(('100 pulses in one trace', np.array([alternating]), Reducer('min_width 1', 10, lead=1, lag=1)))
    out.append(('100 runs, none long enough', np.array([alternating, trace(200, (0, 1), (10, 12), (20, 21), (198, 200))]), Reducer('min_width 2', 10, min_width=2, lead=1, lag=1)))
    out.append(('a plateau peak', np.array([trace(40, (10, 12, 30), (12, 15, 70), (15, 16, 40), (16, 18, 70)), trace(40, (5, 9, 70))]), plain))
    out.append(('windows meet at the stop of the first', np.array([trace(40, (10, 14), (17, 20))]), Reducer('lead = lag = 5', 10, lead=5, lag=5)))
    out.append(('a rejected run between two pulses', np.array([trace(40, (5, 9), (12, 13, 45), (16, 20)), trace(40, (5, 9), (10, 11, 45), (12, 13, 45), (30, 33))]),
                Reducer('min_width 2, wide windows', 10, min_width=2, lead=6, lag=4)))
    # the constant fraction: pedestal 10, y = v - 10
    cfd = []
    cfd.append(trace(8, (2, 3, 15), (3, 4, 19), (4, 5, 14), low=10))                    # s_c == begin (lead 0), a sample below L before it
    cfd.append(trace(8, (1, 2, 13), (2, 3, 15), (3, 4, 19), (4, 5, 14), low=10))        # s_c == begin (lead 0), y(begin - 1) = 3 >= L = 2 at cfd 64
    cfd.append(trace(8, (0, 1, 15), (1, 2, 19), low=10))                               # begin == 0
    cfd.append(trace(8, (2, 3, 4), (3, 4, 30), low=10))                                # y0 negative
    cfd.append(trace(8, (1, 2, 14), (2, 3, 18), low=10))                               # L == y1 at cfd 128: the fraction is 256
    cfd.append(trace(8, (1, 2, 11), (2, 3, 12), (3, 4, 13), low=10))                    # peak 3
    cfd = np.array(cfd)
    for fraction in (128, 64, 256, 1):
        out.append(('constant fraction %d / 256, lead 0' % fraction, cfd, Reducer('cfd %d' % fraction, 1 if fraction == 1 else 4, pedestal=10, cfd=fraction, lag=1)))
        out.append(('constant fraction %d / 256, lead 3' % fraction, cfd, Reducer('cfd %d' % fraction, 1 if fraction == 1 else 4, pedestal=10, cfd=fraction, lead=3, lag=1)))
    base = np.array([np.concatenate(([10, 12, 10, 11], trace(20, (5, 8, 40), low=11))), np.concatenate(([10, 13, 10, 11], trace(20, (5, 8, 40), low=11))),
                     np.concatenate(([10, 10, 60, 60], trace(20, (5, 8, 90), low=11)))]).astype(np.uint16)
    out.append(('a quiet baseline at the spread exactly, a busy one, a pulse in it', base, Reducer('baseline of 4, spread 2', 3, nbaseline=4, baseline_spread=2, lead=1, lag=1)))
    return out


@functools.lru_cache(maxsize=None)
def full_scale():
    """One trace of 65536 samples at full scale -- with pedestal 0, with a baseline of 64 (which then IS full scale: nothing is found)
    and with a baseline of 64 samples of 0 before it: (65536 - 64) * 64 * 65535 > 2^32."""
    everywhere = np.full((1, 65536), 65535, dtype=np.uint16)
    step = everywhere.copy()
    step[0, :64] = 0
    return [('full scale, pedestal 0', everywhere, Reducer('whole trace', 1, lead=65535, lag=65535)),
            ('full scale, baseline of 64', everywhere, Reducer('whole trace, baseline 64', 1, nbaseline=64, lead=65535, lag=65535)),
            ('full scale behind a baseline of 64 zeros', step, Reducer('whole trace, baseline 64', 1, nbaseline=64, lead=65535, lag=65535, cfd=256))]


@functools.lru_cache(maxsize=None)
def random_traces():
    """300 traces of 100 samples: pedestal 200, 0 .. 4 shaped pulses, noise of a few counts."""
    rng = np.random.default_rng(77)
    shape = np.array([0.3, 1.0, 0.8, 0.5, 0.3, 0.15, 0.05])
    adc = np.zeros((300, 100), dtype=np.int64)
    for t in range(300):
        signal = np.zeros(120)
        for _ in range(int(rng.integers(0, 5)) if t % 3 else 0):
            at = int(rng.integers(0, 100))
            signal[at:at + 7] += shape * rng.uniform(10.0, 300.0)
        adc[t] = 200 + np.rint(signal[:100]) + rng.integers(-2, 3, 100)
    return adc.astype(np.uint16), Reducer('random', 8, nbaseline=0, pedestal=200, min_width=2, lead=2, lag=4)


# ---- the calls -------------------------------------------------------------------------------------------------------------------------
def prepare(adc, r, capacity, guard, change=None):
    """The arguments of both calls behind the context, as a dict: the struct, G, ntraces, adc, found_capacity, the ten output arrays
    (sentinel-filled, `guard` entries longer than the call may write) and nfound.  `change`: arguments replaced (None: NULL) and
    fields of the struct ('r.<field>')."""
    change = dict(change or {})
    adc = np.ascontiguousarray(adc, dtype=np.uint16)
    ntraces, G = adc.shape
    v = dict(reducer=r.struct(**{k[2:]: change.pop(k) for k in list(change) if k.startswith('r.')}), G=G, ntraces=ntraces, adc=adc.reshape(-1), found_capacity=capacity)
    for name, kind in PER_TRACE:
        v[name] = np.full(ntraces + (name == 'found_offsets') + guard, SENTINEL32, dtype=np.uint32).view(kind)
    for name, kind in PER_PULSE:
        v[name] = np.full(capacity + guard, SENTINEL64 if kind is np.int64 else SENTINEL32, dtype=np.uint64 if kind is np.int64 else np.uint32).view(kind)
    v['nfound'] = ctypes.c_uint64(SENTINEL_N)
    v.update(change)
    return v


ORDER = ('reducer', 'G', 'ntraces', 'adc', 'found_capacity') + tuple(name for name, _ in PER_TRACE + PER_PULSE) + ('nfound',)


def host_reduce(adc, r, capacity, guard=8, change=None):
    """chroma_daq_reduce_host; (rc, the dict of prepare())."""
    from chroma_amd import _lib
    v = prepare(adc, r, capacity, guard, change)
    args = [None if v[k] is None else _lib.ptr(v[k]) if isinstance(v[k], np.ndarray) else ctypes.byref(v[k]) if isinstance(v[k], (ctypes.Structure, ctypes.c_uint64)) else v[k]
            for k in ORDER]
    return _lib.load().chroma_daq_reduce_host(*args), v


def sentinel(a):
    return SENTINEL64 if a.dtype == np.int64 else SENTINEL32 if a.dtype == np.uint32 else np.uint32(SENTINEL32).view(np.int32)


def untouched(v, names):
    return all((v[name] == sentinel(v[name])).all() for name in names if v[name] is not None)


def assert_reduced(v, want, what, guard=8, filled=True):
    """The per-trace arrays and nfound are the restatement's; with `filled` the per-pulse arrays too, else they are untouched; the
    words behind are."""
    n, total = len(want['trace_base']), len(want['found_start'])
    assert v['nfound'].value == total, '%s: %d found, %d wanted' % (what, v['nfound'].value, total)
    for name, _ in PER_TRACE:
        m = n + (name == 'found_offsets')
        assert len(v[name]) == m + guard and np.array_equal(v[name][:m], want[name]), '%s: %s\n%s\n%s' % (what, name, v[name][:m], want[name])
        assert (v[name][m:] == sentinel(v[name])).all(), '%s: words behind %s' % (what, name)
    for name, _ in PER_PULSE:
        if filled:
            assert np.array_equal(v[name][:total], want[name]), '%s: %s differs at %s\n%s\n%s' % (
                what, name, np.flatnonzero(v[name][:total] != want[name])[:8], v[name][:total][:16], want[name][:16])
            assert (v[name][total:] == sentinel(v[name])).all(), '%s: words behind %s' % (what, name)
        else:
            assert (v[name] == sentinel(v[name])).all(), '%s: %s was touched' % (what, name)


def assert_package(adc, r, want, what):
    """EventTriggers.reduce's arrays (reduce_traces_host on the traces) are the restatement's"""
    from chroma_amd.gpu.daq import reduce_traces_host, FOUND_COLUMNS
    got = reduce_traces_host(adc, r.of_the_package())
    names = [name for name, _ in PER_TRACE] + [name for name, _ in FOUND_COLUMNS]
    assert [name for name, _ in FOUND_COLUMNS] == [name for name, _ in PER_PULSE]
    for name, a in zip(names, got):
        assert a.dtype == (np.int64 if name == 'found_offsets' else dict(PER_TRACE + PER_PULSE)[name]), name
        assert np.array_equal(a, want[name]), '%s: %s' % (what, name)


# ---- 1. the twin and the package are the restatement ---------------------------------------------------------------------------------------
def test_the_host_twin_is_the_restatement_on_the_digitised_trigger_sets():
    seen = dict.fromkeys([r.name for r in reducers()], 0)
    pulses = 0
    for what, adc, r, want in digitised_sets():
        rc, v = host_reduce(adc, r, len(want['found_start']))
        assert rc == 0, what
        assert_reduced(v, want, what)
        seen[r.name] += 1
        pulses += len(want['found_start'])
    assert all(seen.values()) and pulses > 1000, (seen, pulses)          # (every reducer fits some set, and the sets hold pulses)


def test_events_triggers_reduce_is_the_restatement_on_digitised_triggers():
    """Through the package's own path: pulses, trigger, digitize, reduce -- and the per-event slices."""
    from chroma_amd.gpu.daq import DaqTrigger
    from test_daq_digitize_host import SEED, ACQUISITION
    index, which = 1, 4
    name, ps, trig = cases()[index]
    dig = digitisers()[which]
    t = ps.event_pulses().trigger(DaqTrigger(*trig)).digitize(dig.of_the_package(), seed=SEED, acquisition=ACQUISITION)
    assert np.array_equal(t.adc, brute_traces(index, which)[0])
    r = Reducer('pedestal 300', 2, pedestal=300, lead=1, lag=2)
    want = brute_reduce(t.adc, r)
    got = t.reduce(r.of_the_package())
    assert got.reducer == r.of_the_package() and t.reducer is None and t.found_start is None
    for name, kind in PER_TRACE + PER_PULSE:
        assert np.array_equal(getattr(got, name), want[name]) and (name == 'found_offsets' or getattr(got, name).dtype == kind), name
    assert len(got.found_start) > 20
    # event(i) slices them
    total = 0
    for i in range(len(got)):
        e = got.event(i)
        h0, h1 = int(got.hit_offsets[got.offsets[i]]), int(got.hit_offsets[got.offsets[i + 1]])
        f0, f1 = int(want['found_offsets'][h0]), int(want['found_offsets'][h1])
        assert np.array_equal(e.found_offsets, want['found_offsets'][h0:h1 + 1] - f0) and np.array_equal(e.trace_base, want['trace_base'][h0:h1])
        for name, _ in PER_PULSE:
            assert np.array_equal(getattr(e, name), want[name][f0:f1]), name
        total += f1 - f0
        for k in range(len(e)):
            channel, tt, q, npulses, flags = e.reco(k)
            w = e._slice(k)
            counts = np.diff(e.found_offsets[w.start:w.stop + 1])
            assert np.array_equal(channel, e.hit_channel[w][counts > 0]) and np.array_equal(npulses, counts[counts > 0])
            for c, t_c, q_c in zip(channel, tt, q):
                f = e.found(k, c)
                assert len(f) >= 1 and f.t[0] == t_c and abs(f.q.sum() - q_c) <= 1e-9 * abs(q_c)
                first = int(e.bin[k]) - e.trigger.pre
                assert f.t[0] == e.window.t0 + e.window.dt * (first + float(f.time[0]) / 256.0)
                assert np.array_equal(f.q, f.integral.astype(np.float64))          # (N = 1, no gain known)
            dense = e.reco_channels(k)
            assert dense.hit.sum() == len(channel) and np.array_equal(np.flatnonzero(dense.hit), channel)
            assert np.array_equal(dense.t[channel], tt.astype(np.float32)) and np.array_equal(dense.q[channel], q.astype(np.float32))
    assert total == len(want['found_start'])
    with pytest.raises(ValueError, match='hold no traces'):
        ps.event_pulses().trigger(DaqTrigger(*trig)).reduce(r.of_the_package())
    with pytest.raises(ValueError, match='not reduced'):
        t.event(0).reco(0)


@pytest.mark.parametrize('index', range(len(handmade())))
def test_the_host_twin_and_the_package_are_the_restatement_on_the_handmade_traces(index):
    what, adc, r = handmade()[index]
    want = brute_reduce(adc, r)
    rc, v = host_reduce(adc, r, len(want['found_start']))
    assert rc == 0, what
    assert_reduced(v, want, what)
    assert_package(adc, r, want, what)


def made(name):
    for what, adc, r in handmade():
        if what == name:
            return brute_reduce(adc, r)
    raise KeyError(name)


def test_the_handmade_traces_say_what_they_were_made_to_say():
    for G in (1, 2, 63, 64, 65, 128, 129, 200):
        w = made('G = %d: nothing above, everything above, the ends' % G)
        assert list(w['found_offsets']) == ([0, 0, 1, 2, 3, 4] if G <= 2 else [0, 0, 1, 2, 3, 5])          # (G = 2: the two ends are one run)
        assert w['found_flags'][0] == TIME_AT_EDGE | OPEN_AT_START | OPEN_AT_END and w['found_width'][0] == G and w['found_integral'][0] == 50 * G
        assert w['found_flags'][2] & OPEN_AT_END and w['found_start'][2] == G - 1
    w = made('runs over samples 63 / 64')
    assert list(w['found_start']) == [62, 60, 64, 60] and list(w['found_width']) == [4, 4, 6, 10] and w['found_peak_sample'][3] == 64
    assert len(made('100 pulses in one trace')['found_start']) == 100
    w = made('100 runs, none long enough')
    assert list(w['found_offsets']) == [0, 0, 2] and list(w['found_start']) == [10, 198]
    w = made('a plateau peak')
    assert list(w['found_peak_sample']) == [12, 5] and list(w['found_peak']) == [70, 70]
    w = made('windows meet at the stop of the first')
    assert list(w['found_integral']) == [50 * 4, 50 * 3]          # (stop_0 = 17 = a_1: the samples 14 .. 16 are the first pulse's, and are 0)
    w = made('a rejected run between two pulses')
    assert list(w['found_offsets']) == [0, 2, 4] and list(w['found_integral']) == [50 * 4 + 45, 50 * 4, 50 * 4 + 90, 50 * 3]
    w = made('constant fraction 128 / 256, lead 0')
    assert w['found_flags'][0] == 0 and w['found_time'][0] == 256 * 1 + (4 * 256) // 5          # (y(1) = 0 lies before the window)
    assert w['found_flags'][2] == TIME_AT_EDGE | OPEN_AT_START and w['found_time'][2] == 0
    assert w['found_time'][3] == 256 * 2 + ((10 + 6) * 256) // 26
    assert w['found_time'][4] == 256 * 0 + 256 and w['found_flags'][4] == 0
    w = made('constant fraction 64 / 256, lead 0')
    assert w['found_start'][1] == 2 and w['found_flags'][1] == TIME_AT_EDGE and w['found_time'][1] == 256 * 2
    w = made('constant fraction 64 / 256, lead 3')
    assert w['found_flags'][1] == 0 and w['found_time'][1] == 256 * 0 + (2 * 256) // 3
    w = made('constant fraction 256 / 256, lead 3')
    assert list(w['found_time'] - 256 * (w['found_peak_sample'] - 1))[:2] == [256, 256]          # (L = peak: the crossing is the peak sample itself)
    w = made('constant fraction 1 / 256, lead 3')
    assert w['found_peak'][5] == 3 and w['found_time'][5] == 256          # (L = 1 = y(1): fraction 256 from sample 0)
    w = made('a quiet baseline at the spread exactly, a busy one, a pulse in it')
    assert list(w['reduced_flags']) == [0, BASELINE_BUSY, BASELINE_BUSY] and list(w['trace_base']) == [43, 44, 140]
    assert w['found_start'][2] == 2 and w['found_flags'][2] == 0          # (a run among the baseline samples is a run)


@pytest.mark.parametrize('index', range(3))
def test_the_integral_of_a_full_scale_trace_of_65536_samples_needs_its_64_bits(index):
    what, adc, r = full_scale()[index]
    want = brute_reduce(adc, r)
    rc, v = host_reduce(adc, r, 1)
    assert rc == 0
    assert_reduced(v, want, what)
    if index == 0:
        assert want['found_integral'][0] == 65536 * 65535 > 1 << 31 and want['found_flags'][0] == TIME_AT_EDGE | OPEN_AT_START | OPEN_AT_END
    elif index == 1:
        assert len(want['found_start']) == 0 and want['trace_base'][0] == 64 * 65535
    else:
        assert want['found_integral'][0] == (65536 - 64) * 64 * 65535 > 1 << 32 and want['found_peak'][0] == 64 * 65535 and want['found_time'][0] == 64 * 256


def test_the_twin_and_the_package_are_the_restatement_on_300_random_traces():
    adc, r = random_traces()
    want = brute_reduce(adc, r)
    per_trace = np.diff(want['found_offsets'])
    assert (per_trace == 0).sum() >= 50 and (per_trace == 1).sum() >= 20 and (per_trace >= 3).sum() >= 20, np.bincount(per_trace)
    rc, v = host_reduce(adc, r, len(want['found_start']))
    assert rc == 0
    assert_reduced(v, want, 'random traces')
    assert_package(adc, r, want, 'random traces')


# ---- 2. what follows from the definitions, exactly ------------------------------------------------------------------------------------------
def lone_pulse(sample, q, digitizer, reducer):
    """The reduced trace of channel 1 with one pulse of charge count q at sample `sample` of a gate of 64 samples that channel 0 opens."""
    from chroma_amd.gpu.daq import DaqTrigger
    rng = np.random.default_rng(5)
    ps = from_rows(1, 2, 200, [{(0, 20), (1, 12 + sample)}], rng)          # (the gate of the firing at bin 20, pre 8: the bins [12, 76))
    ps.q_int[:] = [1, q]
    t = ps.event_pulses().trigger(DaqTrigger(1, 1, 64, 8, 56)).digitize(digitizer).reduce(reducer)
    assert len(t) == 1 and list(t.event(0).hit_channel) == [0, 1]
    return t.event(0)


def test_the_integral_of_a_lone_pulse_is_the_sum_of_its_taps_and_moving_it_moves_the_time_by_256_per_bin():
    from chroma_amd.gpu.daq import DaqDigitizer, DaqReducer
    digitizer = DaqDigitizer(400.0 * (np.exp(-np.arange(12) / 3.0) - np.exp(-np.arange(12) / 0.7)) + 3.0, pedestal=500, bits=14, shift=16)
    taps, shift, q = [int(x) for x in digitizer.tables(CHARGE_UNIT)[0]], digitizer.shift, 37
    reducer = DaqReducer.for_digitizer(digitizer, 1, lead=12, lag=12)
    assert reducer.pedestal == 500 and reducer.polarity == 1 and reducer.nbaseline == 0 and reducer.gain == digitizer.shape.sum()
    signal = [(q * tap) >> shift for tap in taps]
    assert min(signal) >= 1 and 500 + max(signal) < (1 << 14)          # (one run, no clipping)
    found = {}
    for sample in (13, 14, 20, 40, 51, 58):
        e = lone_pulse(sample, q, digitizer, reducer)
        f = e.found(0, 1)
        assert len(f) == 1, sample
        inside = [signal[d] for d in range(12) if sample + d < 64]
        assert int(f.integral[0]) == sum(inside) and f.start[0] == sample and f.width[0] == len(inside), sample          # (a)
        found[sample] = f
        dt = e.window.dt
    assert found[58].flags[0] == OPEN_AT_END and found[51].flags[0] == 0
    for sample in (14, 20, 40, 51):          # (b): clear of the ends
        f, g = found[13], found[sample]
        k = sample - 13
        assert int(g.time[0]) - int(f.time[0]) == 256 * k and g.t[0] - f.t[0] == pytest.approx(k * dt)
        assert g.start[0] - f.start[0] == k and g.peak_sample[0] - f.peak_sample[0] == k
        for name in ('width', 'peak', 'integral', 'flags'):
            assert getattr(f, name)[0] == getattr(g, name)[0], name
    # the charge in detector units: integral / gain, against the charge that made the pulse
    assert found[20].q[0] == int(found[20].integral[0]) / digitizer.shape.sum() and found[20].q[0] == pytest.approx(q * CHARGE_UNIT, rel=0.02)
    # a falling shape: the same pulse upside down
    falling = DaqDigitizer(-digitizer.shape, pedestal=9000, bits=14, shift=16)
    down = DaqReducer.for_digitizer(falling, 1, lead=12, lag=12)
    assert down.polarity == -1 and down.gain == -digitizer.shape.sum()
    g = lone_pulse(20, q, falling, down).found(0, 1)
    assert len(g) == 1 and g.q[0] > 0 and g.q[0] == pytest.approx(q * CHARGE_UNIT, rel=0.03) and g.start[0] == 20


# ---- 3. refusals, capacities, the package's checks -----------------------------------------------------------------------------------------
def refusals():
    """[(what, change)] of prepare(): every refusal of the header on a small valid call"""
    out = [('polarity 0', {'r.polarity': 0}), ('polarity 2', {'r.polarity': 2}), ('nbaseline 65', {'r.nbaseline': 65}), ('nbaseline beyond G', {'r.nbaseline': 41}),
           ('pedestal 65536', {'r.pedestal': 65536}), ('threshold 0', {'r.threshold': 0}), ('threshold 65536', {'r.threshold': 65536}),
           ('min_width 0', {'r.min_width': 0}), ('min_width 65537', {'r.min_width': 65537}), ('lead 65536', {'r.lead': 65536}), ('lag 65536', {'r.lag': 65536}),
           ('cfd 0', {'r.cfd': 0}), ('cfd 257', {'r.cfd': 257}), ('G 0', {'G': 0}), ('G 65537', {'G': 65537}),
           ('ntraces * G = 2^32', {'G': 65536, 'ntraces': 65536}), ('no reducer', {'reducer': None}), ('no nfound', {'nfound': None})]
    out += [('no %s' % name, {name: None}) for name in ('adc',) + tuple(name for name, _ in PER_TRACE + PER_PULSE)]
    return out


def refusal_case():
    adc = np.array([trace(40, (5, 9), (20, 22)), trace(40), trace(40, (0, 3))])
    return adc, Reducer('threshold 10', 10, lead=2, lag=2), 3          # (found: 3)


def test_the_host_twin_refuses_what_the_header_says_and_writes_nothing():
    adc, r, nfound = refusal_case()
    rc, v = host_reduce(adc, r, nfound)
    assert rc == 0 and v['nfound'].value == nfound
    names = [name for name, _ in PER_TRACE + PER_PULSE]
    for what, change in refusals():
        rc, v = host_reduce(adc, r, nfound, change=change)
        assert rc == ERR_INVALID, what
        assert untouched(v, names) and (v['nfound'] is None or v['nfound'].value == SENTINEL_N), what
    # the pulse arrays may be NULL when there is no room for a pulse anyway
    rc, v = host_reduce(adc[1:2], r, 0, change={name: None for name, _ in PER_PULSE})
    assert rc == 0 and v['nfound'].value == 0 and list(v['found_offsets'][:2]) == [0, 0]


def test_too_little_room_writes_the_count_and_the_per_trace_arrays_and_leaves_the_pulse_arrays():
    adc, r, nfound = refusal_case()
    want = brute_reduce(adc, r)
    assert len(want['found_start']) == nfound
    for capacity in (0, nfound - 1):
        rc, v = host_reduce(adc, r, capacity)
        assert rc == ERR_INVALID, capacity
        assert_reduced(v, want, 'room for %d' % capacity, filled=False)
    rc, v = host_reduce(adc, r, nfound)
    assert rc == 0
    assert_reduced(v, want, 'room for all')


def test_no_traces_is_ok_and_writes_nothing_but_the_count():
    adc, r, nfound = refusal_case()
    for change in ({}, {name: None for name in ('adc',) + tuple(name for name, _ in PER_TRACE + PER_PULSE)}):
        rc, v = host_reduce(adc[:0], r, 4, change=change)
        assert rc == 0 and v['nfound'].value == 0 and untouched(v, [name for name, _ in PER_TRACE + PER_PULSE])


def test_daq_reducer_validates_and_fills_the_struct():
    from chroma_amd import _lib
    from chroma_amd.gpu.daq import DaqReducer, DaqDigitizer
    r = DaqReducer(7, polarity=-1, nbaseline=16, pedestal=3, baseline_spread=5, min_width=2, lead=4, lag=6, cfd=0.25, time_offset_ns=1.5)
    s = r.struct()
    assert [getattr(s, k) for k in FIELDS] == [-1, 16, 3, 5, 7, 2, 4, 6, 64] and r.N == 16 and r.time_offset_ns == 1.5 and r.gain is None
    assert DaqReducer(7).cfd == 128 and DaqReducer(7, cfd=1.0).cfd == 256 and DaqReducer(7, cfd=1 / 256.0).cfd == 1
    assert r == DaqReducer(7, polarity=-1, nbaseline=16, pedestal=3, baseline_spread=5, min_width=2, lead=4, lag=6, cfd=0.25, time_offset_ns=1.5)
    assert hash(r) == hash(DaqReducer.of(r)) and r != DaqReducer(7) and DaqReducer.of(r) is r
    assert DaqReducer.of((9,)) == DaqReducer(9) and DaqReducer.of((9, 2, 3, 0.75, 8, 2)) == DaqReducer(9, lead=2, lag=3, cfd=0.75, nbaseline=8, min_width=2)
    for bad in (dict(threshold=0), dict(threshold=65536), dict(threshold=2.5), dict(threshold='x'), dict(polarity=0), dict(polarity=2), dict(nbaseline=65),
                dict(nbaseline=-1), dict(pedestal=65536), dict(pedestal=-1), dict(baseline_spread=-1), dict(min_width=0), dict(min_width=65537), dict(lead=65536),
                dict(lag=-1), dict(cfd=0.0), dict(cfd=1.01), dict(cfd=float('nan')), dict(cfd='x'), dict(time_offset_ns=float('inf')), dict(gain=0.0)):
        with pytest.raises(ValueError):
            DaqReducer(**dict(dict(threshold=5), **bad))
    for bad in ((), (1, 2), (1, 2, 3, 0.5, 4, 5, 6), 5):
        with pytest.raises(ValueError):
            DaqReducer.of(bad)
    with pytest.raises(ValueError):
        DaqReducer(5, nbaseline=16).check(15)
    with pytest.raises(ValueError):
        DaqReducer(5).check(65537)
    assert DaqReducer(5, nbaseline=16).check(16).nbaseline == 16
    with pytest.raises(ValueError):
        DaqReducer.for_digitizer(DaqDigitizer([1.0], pedestal=-3), 5)          # (no reducer pedestal below 0)
    # the struct's layout is the header's: nine 32-bit words in the order of the table
    assert ctypes.sizeof(_lib.DaqReducer) == 36 and [f[0] for f in _lib.DaqReducer._fields_] == list(FIELDS)
    assert [getattr(_lib.DaqReducer, k).offset for k in FIELDS] == list(range(0, 36, 4))
    import os
    import re
    from conftest import ROOT
    text = open(os.path.join(ROOT, 'include', 'chroma_hip.h')).read()
    body = re.search(r'typedef struct chroma_daq_reducer \{(.*?)\} chroma_daq_reducer;', text, flags=re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    declared = [name.strip() for kind, names in re.findall(r'(int32_t|uint32_t)\s+([^;]+);', body) for name in names.split(',')]
    assert declared == list(FIELDS)


def test_acquire_pulses_simulate_and_chroma_sim_refuse_a_reducer_without_a_digitiser_before_they_touch_a_gpu(capsys):
    from chroma_amd import event, cli
    from chroma_amd.gpu.daq import DaqReducer, GPUEventDaq
    from chroma_amd.sim import Simulation
    daq = object.__new__(GPUEventDaq)          # (no context: anything but the refusal would fail on a missing attribute)
    with pytest.raises(ValueError, match='reducer needs digitizer'):
        daq.acquire_pulses(None, None, [0, 1], (-8.0, 0.5, 70), trigger=(3, 4), reducer=DaqReducer(5))
    sim = object.__new__(Simulation)
    with pytest.raises(ValueError, match='daq_reducer needs daq_digitizer'):
        next(sim.simulate([event.Photons()], run_daq=True, daq_window=(-8.0, 0.5, 64), daq_trigger=(3, 4), daq_reducer=DaqReducer(5)))
    base = ['--daq-window=-8,0.5,512', '--daq-trigger', '2,16,64,8,40']
    digitised = base + ['--daq-digitize', '30,1,6,12,150']
    for argv, message in ((base + ['--daq-reduce', '5'], '--daq-reduce needs --daq-digitize'),
                          (['--daq-reduce', '5'], '--daq-reduce needs --daq-digitize'),
                          (digitised + ['--daq-drop-traces'], '--daq-drop-traces needs --daq-reduce'),
                          (digitised + ['--daq-reduce', '5,2'], '--daq-reduce takes THRESHOLD'),
                          (digitised + ['--daq-reduce', '5,2,2,0.5,4,1,1'], '--daq-reduce takes THRESHOLD'),
                          (digitised + ['--daq-reduce', '0'], '--daq-reduce: a reducer\'s threshold'),
                          (digitised + ['--daq-reduce', '5,2,2,1.5'], '--daq-reduce: a reducer\'s constant fraction'),
                          (digitised + ['--daq-reduce', '5,2,2,0.5,49'], '--daq-reduce: a reducer with a baseline of 49 samples on traces of 48'),
                          (digitised + ['--daq-reduce', 'x'], '--daq-reduce: invalid literal')):
        with pytest.raises(SystemExit):
            cli.main(['@chroma_amd.demo.tiny'] + argv)
        assert message in capsys.readouterr().err, argv
