"""The trigger of the time-binned DAQ on the host: EventPulses.trigger (chroma_amd.gpu.daq.trigger_pulses_host, the NumPy twin of
chroma_daq_trigger_pulses) against a brute-force restatement of the definition in include/chroma_hip.h -- per row and bin the
distinct channels (or the photoelectrons) of the coincidence window, the firing rule bin by bin, the gates, the reduction per
(trigger, channel) -- which shares no code with the package.  Every array is compared exactly, t_first as bits.

The pulse sets are seeded: sparse noise and a few bursts per row, some rows empty, times drawn from a set with negative times,
-0.0 and +0.0.  That they reach the edges (a firing at bin 0 and at the last bin, clipped gates, a sum equal to the threshold, a
re-firing exactly `holdoff` bins on, a pulse in no gate, ...) is ASSERTED on the brute-force result.  tests/test_gpu_daq_trigger.py
runs the same sets through the library.
"""
import functools

import numpy as np
import pytest

NONE = 0xffffffff
NAMES = ('trig_offsets', 'trig_bin', 'trig_sum', 'hit_offsets', 'hit_channel', 'hit_npe', 'hit_q_int', 'hit_t_first', 'hit_flags', 'pulse_trigger')
TIMES = np.array([-7.5, -0.0, 0.0, 1.25, -1e-3, 3.0, 17.0, 250.5, -300.0, 1e-30], dtype=np.float32)

# (nrows, nchannels, nbins, threshold, W, H, pre, post)
SHAPES = [(7, 5, 70, 3, 4, 6, 2, 4), (9, 40, 200, 12, 3, 8, 3, 5), (3, 1, 130, 1, 1, 1, 0, 1), (6, 64, 129, 20, 8, 16, 8, 8),
          (4, 3, 64, 3, 64, 64, 10, 54), (2, 4, 1, 2, 1, 1, 0, 1), (3, 6, 63, 3, 5, 7, 3, 4), (3, 6, 64, 3, 5, 7, 3, 4), (3, 6, 65, 3, 5, 7, 3, 4)]


class PulseSet(object):
    """Pulses in (row, channel, bin) order, as chroma_daq_acquire_pulses writes them."""

    def __init__(self, nrows, nchannels, nbins, offsets, channel, bin, npe, q_int, t_first, flags):
        self.nrows, self.nchannels, self.nbins = nrows, nchannels, nbins
        self.offsets = np.asarray(offsets, dtype=np.uint32)
        self.channel = np.asarray(channel, dtype=np.int32)
        self.bin, self.npe, self.q_int, self.flags = [np.asarray(a, dtype=np.uint32) for a in (bin, npe, q_int, flags)]
        self.t_first = np.asarray(t_first, dtype=np.float32)

    def __len__(self):
        return len(self.channel)

    def columns(self):
        return self.channel, self.bin, self.npe, self.q_int, self.t_first, self.flags

    def event_pulses(self):
        from chroma_amd.gpu.daq import EventPulses, DaqWindow
        return EventPulses(DaqWindow(-8.0, 0.5, self.nbins), self.nchannels, 0.125, self.offsets.astype(np.int64), *self.columns(),
                           outside=np.zeros((self.nrows, 2), dtype=np.uint32))


def from_rows(nrows, nchannels, nbins, rows, rng):
    """rows: per row a set of (channel, bin); the other columns are drawn."""
    rows = [sorted(set(r)) for r in rows]
    n = sum(len(r) for r in rows)
    offsets = np.cumsum([0] + [len(r) for r in rows])
    flat = [cb for r in rows for cb in r]
    return PulseSet(nrows, nchannels, nbins, offsets, [c for c, b in flat], [b for c, b in flat], rng.integers(1, 5, n),
                    rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32) >> rng.integers(0, 20, n).astype(np.uint32),
                    TIMES[rng.integers(0, len(TIMES), n)], np.uint32(1) << rng.integers(0, 12, n).astype(np.uint32))


def random_set(shape, seed):
    """Noise of about one pulse per 12 bins and channel-independent, and bursts of about `threshold` channels over a few bins --
    the first row has one from bin 0 on, the last one in the last bin, rows 1 (and 4) are empty."""
    nrows, nch, nbins, threshold, W, H, pre, post = shape
    rng = np.random.default_rng(seed)
    rows = []
    for r in range(nrows):
        pulses = set()
        if r in (1, 4) and nrows > 2:
            rows.append(pulses)
            continue
        for _ in range(rng.integers(0, max(2, nbins // 12))):
            pulses.add((int(rng.integers(0, nch)), int(rng.integers(0, nbins))))
        starts = [int(rng.integers(0, nbins)) for _ in range(rng.integers(0, 3))]
        if r == 0:
            starts.append(0)
        if r == nrows - 1:
            starts.append(nbins - 1)
        if r == 2 % nrows:
            starts.append(int(nbins // 2))          # a long burst: the sum stays up beyond the lockout
        for k, start in enumerate(starts):
            long = r == 2 % nrows and k == len(starts) - 1
            many = min(nch, threshold + int(rng.integers(0, 3)))
            for c in rng.permutation(nch)[:many]:
                for step in range(2 * H + W if long else 1):
                    b = start + (step if long else int(rng.integers(0, min(W, 2))))
                    if b < nbins:
                        pulses.add((int(c), b))
        rows.append(pulses)
    return from_rows(nrows, nch, nbins, rows, rng)


def wide_set():
    """65536 bins and a handful of pulses, among them bins 0, 32768 and 65535."""
    rng = np.random.default_rng(5)
    rows = [{(0, 0), (1, 0), (2, 1), (0, 32768), (1, 32767), (2, 32768), (3, 40000)}, set(), {(0, 65535), (1, 65535), (3, 65534), (2, 100)}]
    return from_rows(3, 4, 65536, rows, rng)


@functools.lru_cache(maxsize=None)
def cases():
    """[(name, PulseSet, (threshold, W, H, pre, post))], the same for both kinds."""
    out = [('shape %s' % (shape,), random_set(shape, 100 + k), shape[3:]) for k, shape in enumerate(SHAPES)]
    out.append(('65536 bins', wide_set(), (2, 2, 4, 1, 3)))
    return out + handmade()


def handmade():
    rng = np.random.default_rng(9)
    out = []
    # one channel in p, p + 1 and p + W: adjacent and overlapping intervals count once throughout; a second channel from p + 1
    p, W = 10, 4
    out.append(('one channel thrice', from_rows(1, 3, 40, [{(1, p), (1, p + 1), (1, p + W), (2, p + 1)}], rng), (2, W, 30, 0, 1)))
    # a coincidence that straddles bins 63 / 64
    out.append(('coincidence over 63/64', from_rows(2, 4, 130, [{(0, 62), (1, 63), (2, 64), (3, 90)}, {(0, 63), (3, 64), (2, 64)}], rng), (3, 3, 8, 2, 4)))
    # a lockout that straddles them: above threshold from 60 through 70, H = 8: firings at 60 and 68
    out.append(('lockout over 63/64', from_rows(1, 2, 130, [{(c, b) for c in (0, 1) for b in range(60, 71)}], rng), (2, 1, 8, 3, 5)))
    # a gate of 200 bins, one channel in every bin
    out.append(('a gate of 200 bins', from_rows(1, 2, 200, [{(1, b) for b in range(200)}], rng), (1, 1, 200, 0, 200)))
    # everything from the first pulse on in one gate
    nbins = 50
    rows = [{(int(rng.integers(0, 6)), int(rng.integers(3, nbins))) for _ in range(30)}, set(), {(2, 7)}, {(5, 49), (0, 49), (0, 12)}]
    out.append(('one gate per row', from_rows(4, 6, nbins, rows, rng), (1, 1, 2 * nbins, nbins, nbins)))
    return out


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def earliest(times):
    """The smallest of float32 times, -0 below +0."""
    best = times[0]
    for t in times[1:]:
        if t < best or (t == best and np.signbit(t) and not np.signbit(best)):
            best = t
    return best


@functools.lru_cache(maxsize=None)
def brute(index, kind):
    return brute_of(cases()[index][1], kind, *cases()[index][2])


def brute_of(ps, kind, threshold, W, H, pre, post):
    nbins = ps.nbins
    trig_offsets, trig_bin, trig_sum, hit_offsets, hits = [0], [], [], [0], []
    pulse_trigger = np.full(len(ps), NONE, dtype=np.uint32)
    sums = []
    for r in range(ps.nrows):
        lo, hi = int(ps.offsets[r]), int(ps.offsets[r + 1])
        channel, bin = ps.channel[lo:hi], ps.bin[lo:hi].astype(np.int64)
        nxt = 0
        row_sums = np.zeros(nbins, dtype=np.int64)
        for b in (np.unique(np.concatenate([bin + k for k in range(W)])) if nbins > 4096 else range(nbins)):          # (elsewhere the sum is 0)
            if b >= nbins:
                continue
            inside = (bin > b - W) & (bin <= b)
            s = len(np.unique(channel[inside])) if kind == 'nhit' else int(ps.npe[lo:hi][inside].sum())
            row_sums[b] = s
            if s >= threshold and b >= nxt:
                nxt = b + H
                first, last = max(0, b - pre), min(nbins, b + post)
                gate = np.flatnonzero((bin >= first) & (bin < last))
                assert (pulse_trigger[lo + gate] == NONE).all()          # (the gates of a row do not overlap)
                pulse_trigger[lo + gate] = len(trig_bin)
                trig_bin.append(b)
                trig_sum.append(s)
                for c in np.unique(channel[gate]):
                    mine = lo + gate[channel[gate] == c]
                    hits.append((c, int(ps.npe[mine].astype(np.uint64).sum()) & 0xffffffff, int(ps.q_int[mine].astype(np.uint64).sum()) & 0xffffffff,
                                 earliest(ps.t_first[mine]), int(np.bitwise_or.reduce(ps.flags[mine]))))
                hit_offsets.append(len(hits))
        trig_offsets.append(len(trig_bin))
        sums.append(row_sums)
    col = lambda k, dtype: np.array([h[k] for h in hits], dtype=dtype)
    return dict(trig_offsets=np.array(trig_offsets, dtype=np.uint32), trig_bin=np.array(trig_bin, dtype=np.uint32),
                trig_sum=np.array(trig_sum, dtype=np.uint32), hit_offsets=np.array(hit_offsets, dtype=np.uint32),
                hit_channel=col(0, np.int32), hit_npe=col(1, np.uint32), hit_q_int=col(2, np.uint32), hit_t_first=col(3, np.float32),
                hit_flags=col(4, np.uint32), pulse_trigger=pulse_trigger, sums=sums)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def as_dict(t):
    """The arrays of an EventTriggers under the restatement's names."""
    return dict(trig_offsets=t.offsets, trig_bin=t.bin, trig_sum=t.sum, hit_offsets=t.hit_offsets, hit_channel=t.hit_channel, hit_npe=t.hit_npe,
                hit_q_int=t.hit_q_int, hit_t_first=t.hit_t_first, hit_flags=t.hit_flags, pulse_trigger=t.pulse_trigger)


def assert_same(got, want, what):
    for name in NAMES:
        g, w = bits(got[name]), bits(want[name])
        assert len(g) == len(w) and np.array_equal(g.astype(np.int64), w.astype(np.int64)), '%s: %s\n%s\n%s' % (what, name, g, w)


# ---- 1. the twin is the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['nhit', 'npe'])
def test_the_host_trigger_is_the_restatement(kind):
    from chroma_amd.gpu.daq import DaqTrigger, EventTriggers
    for index, (name, ps, (threshold, W, H, pre, post)) in enumerate(cases()):
        want = brute(index, kind)
        got = ps.event_pulses().trigger(DaqTrigger(threshold, W, H, pre, post, kind=kind))
        assert isinstance(got, EventTriggers) and len(got) == ps.nrows
        for name_ in ('bin', 'sum', 'hit_npe', 'hit_q_int', 'hit_flags', 'pulse_trigger'):
            assert getattr(got, name_).dtype == np.uint32, name_
        assert got.hit_channel.dtype == np.int32 and got.hit_t_first.dtype == np.float32
        assert_same(as_dict(got), want, '%s, %s' % (name, kind))


# ---- 2. the inputs reach the edges -----------------------------------------------------------------------------------------------------
def test_the_pulse_sets_reach_the_edges():
    seen = dict.fromkeys(['row without', 'row with several', 'first row', 'last row', 'bin 0', 'last bin', 'clipped at 0', 'clipped at nbins',
                          'sum == threshold', 're-firing after H', 'pulse in no gate', 'trigger without hit'], 0)
    per_shape = []
    for index, (name, ps, (threshold, W, H, pre, post)) in enumerate(cases()[:len(SHAPES) + 1]):
        want = brute(index, 'nhit')
        per_row = np.diff(want['trig_offsets'].astype(np.int64))
        per_shape.append(int(per_row.sum()))
        seen['row without'] += int((per_row == 0).sum())
        seen['row with several'] += int((per_row > 1).sum())
        seen['first row'] += int(per_row[0] > 0)
        seen['last row'] += int(per_row[-1] > 0)
        b = want['trig_bin'].astype(np.int64)
        seen['bin 0'] += int((b == 0).sum())
        seen['last bin'] += int((b == ps.nbins - 1).sum())
        seen['clipped at 0'] += int((b - pre < 0).sum())
        seen['clipped at nbins'] += int((b + post > ps.nbins).sum())
        seen['sum == threshold'] += int((want['trig_sum'] == threshold).sum())
        seen['trigger without hit'] += int((np.diff(want['hit_offsets'].astype(np.int64)) == 0).sum())
        for r in range(ps.nrows):
            mine = b[want['trig_offsets'][r]:want['trig_offsets'][r + 1]]
            seen['re-firing after H'] += int((np.diff(mine) == H).sum())
        seen['pulse in no gate'] += int((want['pulse_trigger'] == NONE).sum())
    print(per_shape, seen)
    assert all(n >= 1 for n in per_shape), per_shape
    del seen['trigger without hit']
    assert all(seen.values()), seen
    for index in range(len(SHAPES) + 1):
        assert len(brute(index, 'npe')['trig_bin']) >= 1


# ---- 3. the hand-made cases say what they were made to say -------------------------------------------------------------------------------
def case(name):
    index = [c[0] for c in cases()].index(name)
    return index, cases()[index][1], cases()[index][2]


def test_one_channel_counts_once():
    index, ps, trig = case('one channel thrice')
    want = brute(index, 'nhit')
    s = want['sums'][0]
    # channel 1 in 10, 11 and 14 (W = 4): up from 10 through 17; channel 2 in 11: up from 11 through 14
    assert s.tolist() == [0] * 10 + [1] + [2] * 4 + [1] * 3 + [0] * 22
    assert want['trig_bin'].tolist() == [11] and want['trig_sum'].tolist() == [2]


def test_coincidence_and_lockout_over_the_wave_edge():
    index, ps, trig = case('coincidence over 63/64')
    want = brute(index, 'nhit')
    assert want['trig_offsets'].tolist() == [0, 1, 2] and want['trig_bin'].tolist() == [64, 64] and want['trig_sum'].tolist() == [3, 3]
    assert want['pulse_trigger'].tolist() == [0, 0, 0, NONE, 1, 1, 1]
    index, ps, trig = case('lockout over 63/64')
    want = brute(index, 'nhit')
    assert want['trig_bin'].tolist() == [60, 68] and (want['sums'][0][60:71] == 2).all()
    # gates [57, 65) and [65, 73): every pulse is in one
    assert want['pulse_trigger'].tolist() == [0] * 5 + [1] * 6 + [0] * 5 + [1] * 6


def test_a_gate_of_200_bins_is_one_hit():
    index, ps, trig = case('a gate of 200 bins')
    want = brute(index, 'nhit')
    assert want['trig_bin'].tolist() == [0] and want['hit_offsets'].tolist() == [0, 1] and want['hit_channel'].tolist() == [1]
    assert want['hit_npe'][0] == ps.npe.sum() and want['hit_q_int'][0] == np.uint32(int(ps.q_int.astype(np.uint64).sum()) & 0xffffffff)
    assert want['hit_flags'][0] == np.bitwise_or.reduce(ps.flags) and want['hit_t_first'][0] == ps.t_first.min() == np.float32(-300.0)
    assert (want['pulse_trigger'] == 0).all() and len(ps) == 200


def test_one_gate_per_row_holds_the_row_from_its_first_pulse_on():
    index, ps, trig = case('one gate per row')
    want = brute(index, 'nhit')
    nonempty = np.flatnonzero(np.diff(ps.offsets.astype(np.int64)))
    assert np.array_equal(np.diff(want['trig_offsets'].astype(np.int64)), (np.diff(ps.offsets.astype(np.int64)) > 0).astype(np.int64))
    k = 0
    for t, r in enumerate(nonempty):
        w = slice(int(ps.offsets[r]), int(ps.offsets[r + 1]))
        assert want['trig_bin'][t] == ps.bin[w].min()
        assert (want['pulse_trigger'][w] == t).all()          # (pre = nbins: the gate reaches back to bin 0)
        for c in np.unique(ps.channel[w]):
            mine = np.flatnonzero(ps.channel[w] == c) + w.start
            assert want['hit_channel'][k] == c and want['hit_npe'][k] == ps.npe[mine].sum()
            assert want['hit_q_int'][k] == np.uint32(int(ps.q_int[mine].astype(np.uint64).sum()) & 0xffffffff)
            k += 1
        assert want['hit_offsets'][t + 1] == k
    assert k == len(want['hit_channel'])


def test_the_minimum_ranks_minus_zero_below_plus_zero():
    from chroma_amd.gpu.daq import DaqTrigger
    rng = np.random.default_rng(1)
    ps = from_rows(1, 1, 8, [{(0, 2), (0, 3)}], rng)
    for times in ([0.0, -0.0], [-0.0, 0.0]):
        ps.t_first = np.array(times, dtype=np.float32)
        want = brute_of(ps, 'nhit', 1, 1, 8, 0, 8)
        got = ps.event_pulses().trigger(DaqTrigger(1, 1, 8, 0, 8))
        assert bits(want['hit_t_first']).tolist() == [0x80000000] and bits(got.hit_t_first).tolist() == [0x80000000]


# ---- 4. classes and refusals --------------------------------------------------------------------------------------------------------------
def test_daq_trigger_validates_and_defaults():
    from chroma_amd.gpu.daq import DaqTrigger, DaqWindow
    t = DaqTrigger(3, 4)
    assert (t.threshold, t.width, t.holdoff, t.pre, t.post, t.kind) == (3, 4, 4, 0, 4, 'nhit')
    t = DaqTrigger(3, 4, pre=2)
    assert (t.holdoff, t.pre, t.post) == (6, 2, 4)
    assert DaqTrigger.of((3, 4, 9, 2, 4)) == DaqTrigger(3, 4, 9, 2, 4) and DaqTrigger.of(t) is t
    assert DaqTrigger.of((3, 4, 9, 2, 4, 'npe')).kind == 'npe' and DaqTrigger.of((3, 4)) == DaqTrigger(3, 4)
    assert DaqTrigger(3, 4).struct().post == 4
    import ctypes
    assert ctypes.sizeof(DaqTrigger(3, 4).struct()) == 24
    for bad in (dict(threshold=0, width=4), dict(threshold=3, width=0), dict(threshold=3, width=4, post=0), dict(threshold=3, width=4, holdoff=5, pre=2, post=4),
                dict(threshold=3, width=4, kind='charge'), dict(threshold=2.5, width=4), dict(threshold=3, width=4, pre=-1), dict(threshold=3, width=1 << 33)):
        with pytest.raises(ValueError):
            DaqTrigger(**bad)
    for bad in (3, (3,), ('a', 4), 'ab', (1, 2, 3, 4, 5, 'nhit', 7)):
        with pytest.raises(ValueError):
            DaqTrigger.of(bad)
    with pytest.raises(ValueError):
        DaqTrigger(3, 65).check(DaqWindow(0.0, 1.0, 64))
    assert DaqTrigger(3, 64).check(DaqWindow(0.0, 1.0, 64)).width == 64
    with pytest.raises(ValueError):
        cases()[0][1].event_pulses().trigger((3, 71))          # (wider than the window of 70 bins)


def test_triggers_of_one_event_and_their_dense_channels():
    from chroma_amd import event
    from chroma_amd.gpu.daq import DaqTrigger, Triggers
    index = 1
    name, ps, (threshold, W, H, pre, post) = cases()[index]
    want = brute(index, 'nhit')
    pulses = ps.event_pulses()
    all_triggers = pulses.trigger(DaqTrigger(threshold, W, H, pre, post))
    unit = np.float32(pulses.charge_unit)
    ntested = 0
    for r in range(ps.nrows):
        t = all_triggers.event(r)
        a, b = int(want['trig_offsets'][r]), int(want['trig_offsets'][r + 1])
        assert isinstance(t, Triggers) and len(t) == b - a
        assert np.array_equal(t.bin, want['trig_bin'][a:b]) and np.array_equal(t.sum, want['trig_sum'][a:b])
        assert t.time.dtype == np.float64 and np.array_equal(t.time, -8.0 + 0.5 * want['trig_bin'][a:b].astype(np.float64))
        of = want['pulse_trigger'][int(ps.offsets[r]):int(ps.offsets[r + 1])]
        assert np.array_equal(t.pulse_trigger, np.where(of == NONE, of, of - np.uint32(a))) and len(t.pulse_trigger) == len(pulses.event(r))
        for k in range(len(t)):
            h = slice(int(want['hit_offsets'][a + k]), int(want['hit_offsets'][a + k + 1]))
            channel, npe, q, t_first, flags = t.sparse(k)
            assert np.array_equal(channel, want['hit_channel'][h]) and np.array_equal(npe, want['hit_npe'][h])
            assert np.array_equal(bits(q), bits((want['hit_q_int'][h].astype(np.float32) * unit).astype(np.float32)))
            dense_t = np.full(ps.nchannels, 1e9, dtype=np.float32)
            dense_q = np.zeros(ps.nchannels, dtype=np.float32)
            dense_f = np.zeros(ps.nchannels, dtype=np.uint32)
            for c, qi, tf, fl in zip(want['hit_channel'][h], want['hit_q_int'][h], want['hit_t_first'][h], want['hit_flags'][h]):
                dense_t[c], dense_q[c], dense_f[c] = tf, np.float32(qi) * unit, fl
            got = t.channels(k)
            assert isinstance(got, event.Channels)
            assert np.array_equal(bits(got.t), bits(dense_t)) and np.array_equal(bits(got.q), bits(dense_q)) and np.array_equal(got.flags, dense_f)
            assert np.array_equal(got.hit, dense_t < 1e8)
            ntested += 1
        with pytest.raises(IndexError):
            t.sparse(len(t))
    assert ntested >= 3
    with pytest.raises(IndexError):
        all_triggers.event(ps.nrows)
    assert event.Event().triggers is None


def test_simulate_refuses_a_trigger_without_a_window_before_it_touches_a_gpu():
    from chroma_amd import event
    from chroma_amd.sim import Simulation
    sim = object.__new__(Simulation)          # (no context, no geometry: anything but the refusal would fail on a missing attribute)
    with pytest.raises(ValueError, match='daq_trigger needs daq_window'):
        next(sim.simulate([event.Photons()], run_daq=True, daq_trigger=(3, 4)))


def test_chroma_sim_refuses_a_trigger_without_a_window(capsys):
    from chroma_amd import cli
    with pytest.raises(SystemExit):
        cli.main(['@chroma_amd.demo.tiny', '--daq-trigger', '3,4'])
    assert '--daq-trigger needs --daq-window' in capsys.readouterr().err
