"""The settings of the time-binned DAQ: ``DaqWindow``, ``DaqNoise``, ``DaqTrigger``, ``DaqDigitizer`` and ``DaqReducer``, each with
the checks of its values, its ``of`` (itself or the one of a tuple) and the C struct or integer tables the library reads; and
``DaqChain``, a readout of them resolved once, over ``DAQ_NEEDS``, the one table of which stage needs which."""
import ctypes

import numpy as np

from chroma_amd import _lib, event
from chroma_amd.gpu.daq.records import count_then_fill, whole


def _padded_cdf(cdf_x, cdf_y):
    """Device CDF tables of len(cdf_x) points each.  Detector._pdf_to_cdf yields a cdf_y that is
    one entry SHORTER than cdf_x (chroma/detector.py:109-112) and the reference then reads
    cdf_y[len(cdf_x)-1] past the end of its device array (chroma/gpu/detector.py:34-36 passes
    len(cdf_x)); here that entry exists and is 1.0, the value a CDF ends with."""
    x = np.asarray(cdf_x, dtype=np.float32)
    y = np.asarray(cdf_y, dtype=np.float32)
    if len(y) < len(x):
        y = np.concatenate([y, np.ones(len(x) - len(y), dtype=np.float32)])
    return x, y[:len(x)]


class _Keyed(object):
    """Settings are equal, and hash alike, when they are of one class and their ``_key()`` is the same."""

    def __eq__(self, other):
        return isinstance(other, type(self)) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())


def _parts(value, sizes, message):
    """``value`` as a tuple of one of the lengths ``sizes``, or ValueError(message)."""
    try:
        parts = tuple(value)
    except TypeError:
        raise ValueError(message)
    if len(parts) not in sizes:
        raise ValueError(message)
    return parts


class DaqWindow(_Keyed):
    """The time axis of a pulse acquisition: ``nbins`` bins of width ``dt`` from ``t0`` on (chroma_daq_window; float32 both, as
    the device bins with them).  A time is in bin ``floor((time - t0) / dt)``, evaluated in float32."""

    def __init__(self, t0, dt, nbins):
        self.t0 = float(np.float32(t0))
        self.dt = float(np.float32(dt))
        self.nbins = int(nbins)
        if not (np.isfinite(self.t0) and np.isfinite(self.dt) and self.dt > 0.0):
            raise ValueError('a DAQ window needs a finite t0 and a finite positive dt')
        if self.nbins != nbins or not 1 <= self.nbins <= 65536:
            raise ValueError('a DAQ window has 1 .. 65536 bins')

    @classmethod
    def of(cls, window):
        """``window`` itself if it is a DaqWindow, or the DaqWindow of a (t0, dt, nbins) triple."""
        if isinstance(window, cls):
            return window
        try:
            t0, dt, nbins = window
        except (TypeError, ValueError):
            raise ValueError('a DAQ window is (t0, dt, nbins)')
        return cls(t0, dt, nbins)

    def bin_edges(self):
        """The nbins + 1 nominal edges t0 + k dt (float64; the device decides a photon's bin by the float32 quotient)."""
        return self.t0 + self.dt * np.arange(self.nbins + 1, dtype=np.float64)

    def struct(self):
        return _lib.DaqWindow(self.t0, self.dt, self.nbins)

    def _key(self):
        return (self.t0, self.dt, self.nbins)

    def __repr__(self):
        return 'DaqWindow(t0=%r, dt=%r, nbins=%d)' % (self.t0, self.dt, self.nbins)


class DaqNoise(object):
    """PMT dark noise for the pulses of a ``DaqWindow`` (chroma_daq_noise): ``rate_hz`` is one dark rate for every channel or
    one per channel, finite and not negative; all-zero rates mean no noise (``off``).  Per (event, channel) the device draws a
    Poisson number of candidates at the LARGEST rate from an integer table and keeps each with probability rate / largest
    rate; a kept one falls uniformly into the window, takes a charge from the detector's charge CDF and carries ``flag`` as
    its history (include/chroma_hip.h, "dark noise").

    ``tables`` builds the integer tables in float64.  With mu = max(rate) * 1e-9 * nbins * dt (dt in ns) the expected
    candidates per (event, channel), the count table holds floor(P(X <= j) * 2^32) up to the first entry that saturates at
    2^32 - 1, and it has 64 entries at most: that holds up to mu = 25.976 (where P(X > 63) passes 2^-32), so every mu up to
    ``MAX_MU`` = 25.9 has its table and from mu = 26 on ``tables`` raises ValueError -- take a shorter window."""

    MAX_COUNT = 64
    MAX_MU = 25.9

    def __init__(self, rate_hz, flag=event.DARK_NOISE):
        rate = np.asarray(rate_hz, dtype=np.float64)
        if rate.ndim > 1 or rate.size < 1 or not np.isfinite(rate).all() or (rate < 0).any():
            raise ValueError('dark rates: a finite rate that is not negative, or one per channel')
        self.rate_hz = rate
        self.flag = int(flag)
        if self.flag != flag or not 0 < self.flag <= 0xffffffff or self.flag & (self.flag - 1):
            raise ValueError('the flag of the noise is one history bit')
        self.off = not (rate > 0).any()

    @classmethod
    def of(cls, noise):
        """``noise`` itself if it is a DaqNoise, or the DaqNoise of a rate (or of the rates per channel)."""
        return noise if isinstance(noise, cls) else cls(noise)

    def mu(self, window):
        """The expected candidates per (event, channel): the largest rate over the whole window."""
        window = DaqWindow.of(window)
        return float(self.rate_hz.max()) * 1e-9 * window.nbins * window.dt

    def tables(self, window, nchannels):
        """(count_cdf, accept): the uint32 arrays of chroma_daq_noise for ``window`` and a detector of ``nchannels``."""
        nchannels = int(nchannels)
        if self.rate_hz.ndim == 1 and len(self.rate_hz) != nchannels:
            raise ValueError('%d dark rates for %d channels' % (len(self.rate_hz), nchannels))
        if self.off:
            raise ValueError('no channel has a dark rate: there are no tables (DaqNoise.off)')
        mu = self.mu(window)
        top = float(self.rate_hz.max())
        p = np.exp(-mu)
        total = 0.0
        cdf = []
        for j in range(self.MAX_COUNT):
            total += p
            entry = min(int(np.floor(total * 2.0 ** 32)), 2 ** 32 - 1)
            cdf.append(entry)
            if entry == 2 ** 32 - 1:
                break
            p = p * mu / (j + 1)
        else:
            raise ValueError('mu = %g candidates per channel and event: more than a table of %d entries holds (mu <= %g)' % (mu, self.MAX_COUNT, self.MAX_MU))
        accept = np.floor(np.broadcast_to(self.rate_hz, (nchannels,)) / top * 2.0 ** 31 + 0.5).astype(np.uint32)
        return np.array(cdf, dtype=np.uint32), accept

    def sample(self, window, nrows, nchannels, charge_cdf, charge_unit, seed=0, acquisition=0):
        """The kept noise photoelectrons of ``nrows`` events on the HOST (chroma_daq_noise_host: no GPU), bit for bit what
        ``GPUEventDaq.acquire_pulses(noise=self, acquisition=acquisition)`` mixes into the pulses of a context seeded with ``seed``:
        a structured array of (row, channel, bin, time, charge_int) in (row, channel, candidate) order.  ``charge_cdf``: the (x, y)
        of the detector's charge CDF as the DAQ holds it; ``charge_unit``: its charge unit."""
        window = DaqWindow.of(window)
        dtype = [('row', np.uint32), ('channel', np.uint32), ('bin', np.uint32), ('time', np.float32), ('charge_int', np.uint32)]
        if self.off:
            return np.zeros(0, dtype=dtype)
        lib = _lib.load()
        count_cdf, accept = self.tables(window, nchannels)
        qx, qy = _padded_cdf(*charge_cdf)
        qx, qy = np.ascontiguousarray(qx), np.ascontiguousarray(qy)
        tables = _lib.DaqTables(None, None, 0, _lib.ptr(qx), _lib.ptr(qy), len(qx), float(charge_unit))
        win = window.struct()
        struct = _lib.DaqNoise(_lib.ptr(count_cdf), len(count_cdf), _lib.ptr(accept), self.flag)
        n = ctypes.c_uint64(0)
        columns = []

        def call(capacity):
            columns[:] = [np.zeros(capacity, dtype=np.uint32) for _ in dtype]          # (words: the times come back as their bits)
            rc = lib.chroma_daq_noise_host(ctypes.byref(tables), ctypes.byref(win), ctypes.byref(struct), int(nrows), int(nchannels),
                                           int(seed), int(acquisition) & 0xffffffff, capacity,
                                           *([_lib.ptr(a) if capacity else None for a in columns] + [ctypes.byref(n)]))
            return rc, n.value
        count_then_fill(call, 0)
        out = np.zeros(int(n.value), dtype=dtype)
        for (name, kind), a in zip(dtype, columns):
            out[name] = a[:len(out)].view(kind)
        return out


class DaqTrigger(_Keyed):
    """A trigger on the pulses of a ``DaqWindow`` (chroma_daq_trigger; everything in BINS of the window).  The sum S(b) of a bin
    is over the pulses of the bins (b - width, b]: the number of distinct channels among them (``kind='nhit'``) or their
    photoelectrons (``'npe'``).  Through the bins ascending the trigger fires at b if S(b) >= threshold and b is not within
    ``holdoff`` bins behind the last firing; the gate of a firing is the bins [b - pre, b + post), clipped to the window.
    Defaults: ``post = width`` and ``holdoff = pre + post`` (the smallest allowed: the gates of an event never overlap)."""

    KINDS = {'nhit': 0, 'npe': 1}

    def __init__(self, threshold, width, holdoff=None, pre=0, post=None, kind='nhit'):
        if kind not in self.KINDS:
            raise ValueError("a DAQ trigger's kind is 'nhit' or 'npe'")
        self.kind = kind
        for name, value in (('threshold', threshold), ('width', width), ('pre', pre), ('post', width if post is None else post), ('holdoff', holdoff)):
            if name == 'holdoff' and value is None:
                value = self.pre + self.post
            setattr(self, name, whole(value, 0, 0xffffffff, 'a DAQ trigger\'s %s is a whole number of bins' % name,
                                      'a DAQ trigger\'s %s is a whole number of 32 bits' % name))
        if self.threshold < 1 or self.width < 1 or self.post < 1:
            raise ValueError('a DAQ trigger needs a threshold, a width and a post of at least 1')
        if self.holdoff < max(1, self.pre + self.post):
            raise ValueError('a DAQ trigger needs holdoff >= max(1, pre + post): the gates of an event do not overlap')

    @classmethod
    def of(cls, trigger):
        """``trigger`` itself if it is a DaqTrigger, or the DaqTrigger of a (threshold, width[, holdoff, pre, post[, kind]]) tuple."""
        if isinstance(trigger, cls):
            return trigger
        return cls(*_parts(trigger, range(2, 7), 'a DAQ trigger is (threshold, width[, holdoff, pre, post[, kind]])'))

    def check(self, window):
        """Raises ValueError unless the trigger fits ``window`` (a coincidence window of at most its bins)."""
        if self.width > window.nbins:
            raise ValueError('a DAQ trigger of width %d on a window of %d bins' % (self.width, window.nbins))
        return self

    def struct(self):
        return _lib.DaqTrigger(self.KINDS[self.kind], self.threshold, self.width, self.holdoff, self.pre, self.post)

    def _key(self):
        return (self.kind, self.threshold, self.width, self.holdoff, self.pre, self.post)

    def __repr__(self):
        return 'DaqTrigger(threshold=%d, width=%d, holdoff=%d, pre=%d, post=%d, kind=%r)' % (
            self.threshold, self.width, self.holdoff, self.pre, self.post, self.kind)


CLIPPED_HIGH, CLIPPED_LOW = 1, 2          # the bits of a trace's flag word: some sample clipped at the top, some at 0


class DaqDigitizer(_Keyed):
    """The digitiser of a trigger's gates (chroma_daq_digitizer): every gated (firing, channel) is read out as a trace of
    ``pre + post`` ADC samples, one per bin from ``pre`` bins before the firing on.  ``shape`` is the response to one unit of the
    detector's charge, in ADC counts per bin from the pulse's own bin on (1 .. 1024 bins; it may be negative); pulses pile up, and
    pulses from before the gate have their tails in it.  ``pedestal`` (ADC counts) is added, then electronics noise -- a Gaussian
    of ``noise_sigma`` ADC counts rounded to whole counts, one draw per (event, channel, bin) whichever firing reads it -- and the
    sample is clipped to ``bits`` bits; ``trace_flags`` says where that happened (``CLIPPED_HIGH``, ``CLIPPED_LOW``).  The
    arithmetic is fixed point with ``shift`` fractional bits (include/chroma_hip.h, "digitiser").

    ``tables`` builds the integer tables in float64: tap d = round(shape[d] * charge_unit * 2^shift), the response to one charge
    COUNT, and for the noise ``noise_lo = -32`` and 64 entries floor(Phi((noise_lo + j + 0.5) / sigma) * 2^32), saturated at
    2^32 - 1 -- every sigma up to ``MAX_SIGMA`` = 8 out to 4 sigma."""

    MAX_TAPS = 1024
    MAX_NOISE = 64
    NOISE_LO = -32
    MAX_SIGMA = 8.0

    def __init__(self, shape, pedestal=0, bits=14, shift=16, noise_sigma=0.0):
        shape = np.array(shape, dtype=np.float64)
        if shape.ndim != 1 or not 1 <= len(shape) <= self.MAX_TAPS or not np.isfinite(shape).all():
            raise ValueError('a digitiser\'s shape is 1 .. %d finite values' % self.MAX_TAPS)
        shape.setflags(write=False)
        self.shape = shape
        for name, value, lo, hi in (('pedestal', pedestal, -2 ** 31, 2 ** 31 - 1), ('bits', bits, 1, 16), ('shift', shift, 0, 31)):
            setattr(self, name, whole(value, lo, hi, 'a digitiser\'s %s is a whole number' % name,
                                      'a digitiser\'s %s is a whole number of %d .. %d' % (name, lo, hi)))
        self.noise_sigma = float(noise_sigma)
        if not 0.0 <= self.noise_sigma <= self.MAX_SIGMA:
            raise ValueError('a digitiser\'s noise has a sigma of 0 .. %g ADC counts: the table holds no more' % self.MAX_SIGMA)

    @classmethod
    def biexponential(cls, amplitude, rise_ns, fall_ns, dt, length=None, **kw):
        """The digitiser whose shape is exp(-t / fall_ns) - exp(-t / rise_ns), scaled so that the curve peaks at ``amplitude``
        ADC counts per unit charge, sampled at the centres t = (d + 0.5) dt of the bins (``dt`` in ns) from the pulse's own on.
        ``length`` bins; by default up to where the curve has fallen to a thousandth of its peak, 1024 at the most."""
        amplitude, rise, fall, dt = float(amplitude), float(rise_ns), float(fall_ns), float(dt)
        if not (0.0 < rise < fall < float('inf')) or not (0.0 < dt < float('inf')) or not np.isfinite(amplitude):
            raise ValueError('a biexponential pulse needs 0 < rise_ns < fall_ns, a positive dt and a finite amplitude')
        t_peak = np.log(fall / rise) * rise * fall / (fall - rise)
        peak = np.exp(-t_peak / fall) - np.exp(-t_peak / rise)
        if length is None:
            length = int(min(cls.MAX_TAPS, max(1, np.ceil((t_peak + fall * np.log(1000.0)) / dt))))
        if int(length) != length or not 1 <= int(length) <= cls.MAX_TAPS:
            raise ValueError('a digitiser\'s shape has 1 .. %d bins' % cls.MAX_TAPS)
        t = (np.arange(int(length), dtype=np.float64) + 0.5) * dt
        return cls(amplitude * (np.exp(-t / fall) - np.exp(-t / rise)) / peak, **kw)

    @classmethod
    def of(cls, digitizer):
        """``digitizer`` itself if it is a DaqDigitizer, or the biexponential one of an (amplitude, rise_ns, fall_ns, dt[, bits[,
        pedestal[, sigma]]]) tuple."""
        if isinstance(digitizer, cls):
            return digitizer
        message = 'a DAQ digitiser is (amplitude, rise_ns, fall_ns, dt[, bits[, pedestal[, sigma]]])'
        parts = _parts(digitizer, range(4, 8), message)
        kw = dict(zip(('bits', 'pedestal', 'noise_sigma'), parts[4:]))
        try:
            return cls.biexponential(*[float(x) for x in parts[:4]], **kw)
        except TypeError:
            raise ValueError(message)

    def check(self, trigger):
        """Raises ValueError unless ``trigger``'s gate is one this digitiser can read: pre + post of 65536 samples at the most."""
        if trigger.pre + trigger.post > 65536:
            raise ValueError('a gate of %d samples: a trace holds 65536' % (trigger.pre + trigger.post))
        return self

    def tables(self, charge_unit):
        """(taps int32, noise_cdf uint32 -- empty without noise --, noise_lo) of chroma_daq_digitizer for a detector whose
        charge counts are of ``charge_unit``."""
        charge_unit = float(charge_unit)
        if not (0.0 < charge_unit < float('inf')):
            raise ValueError('a charge unit is finite and positive')
        taps = np.rint(self.shape * charge_unit * 2.0 ** self.shift)
        if not np.isfinite(taps).all() or (taps > 2 ** 31 - 1).any() or (taps < -2 ** 31).any():
            raise ValueError('the taps do not fit 32 bits: a smaller shift, or a smaller shape')
        cdf = np.zeros(0, dtype=np.uint32)
        if self.noise_sigma > 0.0:
            import math
            x = (self.NOISE_LO + np.arange(self.MAX_NOISE, dtype=np.float64) + 0.5) / self.noise_sigma
            phi = np.array([0.5 * (1.0 + math.erf(v / math.sqrt(2.0))) for v in x], dtype=np.float64)
            cdf = np.minimum(np.floor(phi * 2.0 ** 32), 2.0 ** 32 - 1).astype(np.uint32)
        return taps.astype(np.int32), cdf, self.NOISE_LO

    def struct(self, charge_unit):
        """(the chroma_daq_digitizer, the host arrays it points to: keep them alive as long as it is used)"""
        taps, cdf, lo = self.tables(charge_unit)
        return _lib.DaqDigitizer(_lib.ptr(taps), len(taps), self.shift, self.pedestal, self.bits, _lib.ptr(cdf) if len(cdf) else None,
                                 len(cdf), lo), (taps, cdf)

    def _key(self):
        return (self.shape.tobytes(), self.pedestal, self.bits, self.shift, self.noise_sigma)

    def __repr__(self):
        return 'DaqDigitizer(shape=<%d bins, peak %g>, pedestal=%d, bits=%d, shift=%d, noise_sigma=%r)' % (
            len(self.shape), float(np.abs(self.shape).max()), self.pedestal, self.bits, self.shift, self.noise_sigma)


TIME_AT_EDGE, OPEN_AT_START, OPEN_AT_END = 1, 2, 4          # the bits of a found pulse's flag word
BASELINE_BUSY = 1                                           # the bit of a reduced trace's flag word


class DaqReducer(_Keyed):
    """The reduction of digitised traces (chroma_daq_reducer): what the electronics make of a trace -- the pulses in it, the
    charge of each and a constant-fraction time.  The baseline is the mean of the first ``nbaseline`` samples (0 .. 64), or
    ``pedestal`` when that is 0 (``BASELINE_BUSY`` when they spread by more than ``baseline_spread`` counts); a pulse is
    ``min_width`` or more consecutive samples ``threshold`` ADC counts or more above it (below, with ``polarity=-1``), integrated from
    ``lead`` samples before to ``lag`` samples behind it but never into a neighbour's window, and timed where its leading edge
    crosses the fraction ``cfd`` (1/256 .. 1) of its peak, interpolated to 1/256 of a sample.  The arithmetic is integer
    (include/chroma_hip.h, "trace reduction").

    ``time_offset_ns`` is subtracted from the times ``Triggers.found`` and ``reco`` give (the shape's rise to the fraction);
    ``gain``, ADC counts x bins per unit of the detector's charge (``for_digitizer``: the sum of the shape), turns integrals into
    charges."""

    def __init__(self, threshold, polarity=1, nbaseline=0, pedestal=0, baseline_spread=0, min_width=1, lead=0, lag=0, cfd=0.5, time_offset_ns=0.0,
                 gain=None):
        ranges = (('threshold', threshold, 1, 65535), ('polarity', polarity, -1, 1), ('nbaseline', nbaseline, 0, 64), ('pedestal', pedestal, 0, 65535),
                  ('baseline_spread', baseline_spread, 0, 0xffffffff), ('min_width', min_width, 1, 65536), ('lead', lead, 0, 65535), ('lag', lag, 0, 65535))
        for name, value, lo, hi in ranges:
            no_fit = 'a reducer\'s %s is a whole number of %d .. %d%s' % (name, lo, hi, ', not 0' if name == 'polarity' else '')
            setattr(self, name, whole(value, lo, hi, 'a reducer\'s %s is a whole number' % name, no_fit))
            if name == 'polarity' and self.polarity == 0:
                raise ValueError(no_fit)
        try:
            fraction = float(cfd)
        except (TypeError, ValueError):
            raise ValueError('a reducer\'s constant fraction is a number')
        if not (fraction == fraction) or not 1 <= int(round(fraction * 256)) <= 256:
            raise ValueError('a reducer\'s constant fraction is 1/256 .. 1')
        self.cfd = int(round(fraction * 256))          # in 1/256
        self.time_offset_ns = float(time_offset_ns)
        self.gain = None if gain is None else float(gain)
        if not np.isfinite(self.time_offset_ns) or (self.gain is not None and not (np.isfinite(self.gain) and self.gain != 0.0)):
            raise ValueError('a reducer\'s time offset is finite, its gain finite and not 0')

    @classmethod
    def for_digitizer(cls, digitizer, threshold, **kw):
        """The reducer that fits ``digitizer``'s traces: the polarity of its shape's largest excursion, its pedestal, and
        ``gain = sum(shape)``, ADC counts x bins per unit charge."""
        shape = digitizer.shape
        kw.setdefault('polarity', 1 if shape[int(np.argmax(np.abs(shape)))] >= 0.0 else -1)
        kw.setdefault('pedestal', digitizer.pedestal)
        gain = float(shape.sum())
        kw.setdefault('gain', gain if gain != 0.0 else None)
        return cls(threshold, **kw)

    @classmethod
    def of(cls, reducer):
        """``reducer`` itself if it is a DaqReducer, or the one of a (threshold[, lead, lag[, cfd[, nbaseline[, min_width]]]]) tuple."""
        if isinstance(reducer, cls):
            return reducer
        parts = _parts(reducer, (1, 3, 4, 5, 6), 'a DAQ reducer is (threshold[, lead, lag[, cfd[, nbaseline[, min_width]]]])')
        return cls(parts[0], **dict(zip(('lead', 'lag', 'cfd', 'nbaseline', 'min_width'), parts[1:])))

    def check(self, G):
        """Raises ValueError unless traces of ``G`` samples can be reduced: 1 .. 65536 of them, the baseline's at least."""
        if not 1 <= G <= 65536 or self.nbaseline > G:
            raise ValueError('a reducer with a baseline of %d samples on traces of %d: traces have 1 .. 65536 samples, the baseline\'s at least' % (self.nbaseline, G))
        return self

    @property
    def N(self):
        """What ``found_integral`` and ``found_peak`` are scaled by: max(nbaseline, 1)."""
        return max(self.nbaseline, 1)

    def struct(self):
        return _lib.DaqReducer(self.polarity, self.nbaseline, self.pedestal, self.baseline_spread, self.threshold, self.min_width, self.lead, self.lag, self.cfd)

    def _key(self):
        return (self.threshold, self.polarity, self.nbaseline, self.pedestal, self.baseline_spread, self.min_width, self.lead, self.lag, self.cfd,
                self.time_offset_ns, self.gain)

    def __repr__(self):
        return ('DaqReducer(threshold=%d, polarity=%d, nbaseline=%d, pedestal=%d, baseline_spread=%d, min_width=%d, lead=%d, lag=%d, cfd=%d/256, '
                'time_offset_ns=%r, gain=%r)' % (self.threshold, self.polarity, self.nbaseline, self.pedestal, self.baseline_spread, self.min_width,
                                                self.lead, self.lag, self.cfd, self.time_offset_ns, self.gain))


# which stage of a readout reads what another made: (stage, the stage it needs), in the order the stages run
DAQ_NEEDS = (('trigger', 'window'), ('noise', 'window'), ('digitizer', 'trigger'), ('reducer', 'digitizer'), ('seeder', 'trigger'),
             ('direction', 'seeder'))


def daq_needs(given, names=None, stages=None, reasons=None):
    """Raises ValueError for the first of ``stages`` (default: all of ``DAQ_NEEDS``, in its order) that is given without the stage it
    needs.  ``given``: stage -> its value, None or absent for a stage that is not asked for; ``names``: stage -> what the caller
    calls it (default: the stage itself); ``reasons``: stage -> what the caller puts in front of that stage's message."""
    needs = dict(DAQ_NEEDS)
    name = (lambda stage: stage) if names is None else names.__getitem__
    for stage in (needs if stages is None else stages):
        if given.get(stage) is not None and given.get(needs[stage]) is None:
            raise ValueError('%s%s needs %s' % ((reasons or {}).get(stage, ''), name(stage), name(needs[stage])))


class DaqChain(object):
    """A readout, resolved: ``window`` (a DaqWindow), ``trigger``, ``noise`` (None also for noise that is ``off``), ``digitizer``,
    ``reducer`` -- each None or its settings object, converted (``of``) and checked against the stage it reads exactly once, here --
    and ``keep_traces``.  ``nchannels``, where it is known: the noise's tables have to fit the window and that many channels."""

    def __init__(self, window, trigger=None, noise=None, digitizer=None, reducer=None, keep_traces=True, nchannels=None):
        daq_needs(dict(window=window, trigger=trigger, noise=noise, digitizer=digitizer, reducer=reducer))
        self.window = DaqWindow.of(window)
        self.trigger = None if trigger is None else DaqTrigger.of(trigger).check(self.window)
        noise = None if noise is None else DaqNoise.of(noise)
        if noise is not None and not noise.off and nchannels is not None:
            noise.tables(self.window, nchannels)          # (raises what does not fit the window or the detector)
        self.noise = None if noise is None or noise.off else noise
        self.digitizer = None if digitizer is None else DaqDigitizer.of(digitizer).check(self.trigger)
        self.reducer = None if reducer is None else DaqReducer.of(reducer).check(self.trigger.pre + self.trigger.post)
        self.keep_traces = keep_traces
