"""The PDF layer's semantics on the host (reference: chroma/cuda/pdf.cu, chroma/gpu/pdf.py, chroma/likelihood.py).

A NaN time, and in the (time, charge) paths a NaN charge, is "not hit" in every restatement (the window tests are written
in the positive form), and a NaN event time gives no nearest-distance candidate: DESIGN.md 3.6.  On every input without
a NaN the restatements are the reference's (tests/test_ref_pdf_host.py holds them to its own pdf.cu).

Each device kernel is restated twice in NumPy: as the obvious per-channel loop of the reference, and vectorised.  The
two agree here on small random cases, and tests/test_gpu_pdf.py holds the device to them.  Also: the host arithmetic of
get_pdf_eval / compute_bandwidth, the NLL of Likelihood against a stub simulation, and the ``chroma`` alias."""
import math

import numpy as np
import pytest

F = np.float32
NOT_HIT = F(1e9)


def _copy(a, i, stride, nchannels):
    return a[i * stride:i * stride + nchannels]


def _charge_uint(qf):
    qf = np.asarray(qf, dtype=np.float32)
    out = np.zeros(qf.shape, dtype=np.float64)
    pos = qf > 0
    out[pos] = np.minimum(np.floor(qf[pos].astype(np.float64)), 4294967295.0)
    return out.astype(np.uint32)


# ---- bin_hits (pdf.cu:9-32, bin indices clamped) ----------------------------------------------------------------
def bin_hits_loop(t, q, nchannels, ndaq, stride, tbins, trange, qbins, qrange, hitcount=None, pdf=None):
    tmin, tmax, qmin, qmax = F(trange[0]), F(trange[1]), F(qrange[0]), F(qrange[1])
    hitcount = np.zeros(nchannels, np.uint32) if hitcount is None else hitcount.copy()
    pdf = np.zeros((nchannels, tbins, qbins), np.uint32) if pdf is None else pdf.copy()
    for c in range(nchannels):
        for i in range(ndaq):
            tt, qf = F(t[i * stride + c]), F(q[i * stride + c])
            qu = 0 if not qf > 0 else (4294967295 if qf >= 4294967296.0 else int(qf))
            qq = F(qu)
            if tt < F(1e8) and tt >= tmin and tt < tmax and qq >= qmin and qq < qmax:
                hitcount[c] += 1
                tbin = min(max(int((tt - tmin) / (tmax - tmin) * F(tbins)), 0), tbins - 1)
                qbin = min(max(int((qq - qmin) / (qmax - qmin) * F(qbins)), 0), qbins - 1)
                pdf[c, tbin, qbin] += 1
    return hitcount, pdf


def bin_hits_vec(t, q, nchannels, ndaq, stride, tbins, trange, qbins, qrange, hitcount=None, pdf=None):
    tmin, tmax, qmin, qmax = F(trange[0]), F(trange[1]), F(qrange[0]), F(qrange[1])
    hitcount = np.zeros(nchannels, np.uint32) if hitcount is None else hitcount.copy()
    pdf = np.zeros((nchannels, tbins, qbins), np.uint32) if pdf is None else pdf.copy()
    T = np.asarray(t, np.float32)[:ndaq * stride].reshape(ndaq, stride)[:, :nchannels] if len(t) >= ndaq * stride else \
        np.stack([_copy(t, i, stride, nchannels) for i in range(ndaq)])
    Q = np.stack([_copy(np.asarray(q, np.float32), i, stride, nchannels) for i in range(ndaq)])
    QQ = _charge_uint(Q).astype(np.float32)
    ok = (T < F(1e8)) & (T >= tmin) & (T < tmax) & (QQ >= qmin) & (QQ < qmax)
    ch = np.broadcast_to(np.arange(nchannels), T.shape)[ok]
    tb = np.clip(((T[ok] - tmin) / (tmax - tmin) * F(tbins)).astype(np.int64), 0, tbins - 1)
    qb = np.clip(((QQ[ok] - qmin) / (qmax - qmin) * F(qbins)).astype(np.int64), 0, qbins - 1)
    hitcount += np.bincount(ch, minlength=nchannels).astype(np.uint32)
    np.add.at(pdf, (ch, tb, qb), 1)
    return hitcount, pdf


# ---- accumulate_bincount + accumulate_nearest_neighbor (pdf.cu:34-219) -------------------------------------------
def eval_accumulate_loop(event_hit, event_time, mc_time, nchannels, ndaq, stride, min_twidth, trange, k, state=None):
    """state = (hitcount, bincount, nearest[nchannels, k]); returns the new state."""
    tmin, tmax = F(trange[0]), F(trange[1])
    half = F(min_twidth) * F(0.5)
    if state is None:
        state = (np.zeros(nchannels, np.uint32), np.zeros(nchannels, np.uint32), np.full((nchannels, k), NOT_HIT, np.float32))
    hitcount, bincount, nearest = (a.copy() for a in state)
    for c in range(nchannels):
        cands = []
        for i in range(ndaq):
            mc = F(mc_time[i * stride + c])
            if not (mc < F(1e8) and mc >= tmin and mc <= tmax):          # a NaN time is not a hit
                continue
            hitcount[c] += 1
            if not event_hit[c]:
                continue
            d = F(abs(mc - F(event_time[c])))
            if d < half:
                bincount[c] += 1
            if bincount[c] < k and d == d:          # a NaN distance (NaN event time) is no candidate
                cands.append(d)
        if cands:
            nearest[c] = np.sort(np.concatenate([nearest[c], np.array(cands, np.float32)]))[:k]
    return hitcount, bincount, nearest


def eval_accumulate_vec(event_hit, event_time, mc_time, nchannels, ndaq, stride, min_twidth, trange, k, state=None):
    tmin, tmax = F(trange[0]), F(trange[1])
    half = F(min_twidth) * F(0.5)
    if state is None:
        state = (np.zeros(nchannels, np.uint32), np.zeros(nchannels, np.uint32), np.full((nchannels, k), NOT_HIT, np.float32))
    hitcount, bincount, nearest = (a.copy() for a in state)
    hit = np.asarray(event_hit).astype(bool)
    M = np.stack([_copy(np.asarray(mc_time, np.float32), i, stride, nchannels) for i in range(ndaq)])
    valid = (M < F(1e8)) & (M >= tmin) & (M <= tmax)
    hitcount += valid.sum(axis=0).astype(np.uint32)
    D = np.abs(M - np.asarray(event_time, np.float32)[None, :])
    inbin = valid & (D < half) & hit[None, :]
    running = bincount[None, :].astype(np.int64) + np.cumsum(inbin, axis=0)
    cand = valid & hit[None, :] & (running < k) & ~np.isnan(D)
    bincount += inbin.sum(axis=0).astype(np.uint32)
    merged = np.sort(np.concatenate([nearest.T, np.where(cand, D, np.float32(np.inf))], axis=0), axis=0)[:k]
    nearest = np.ascontiguousarray(merged.T)
    return hitcount, bincount, nearest


# ---- accumulate_moments (pdf.cu:223-265) -------------------------------------------------------------------
def moments_loop(t, q, nchannels, ndaq, stride, trange, qrange, time_only=True, state=None):
    tmin, tmax, qmin, qmax = F(trange[0]), F(trange[1]), F(qrange[0]), F(qrange[1])
    if state is None:
        state = (np.zeros(nchannels, np.uint32),) + tuple(np.zeros(nchannels, np.float32) for _ in range(4))
    m0, t1, t2, q1, q2 = (a.copy() for a in state)
    for c in range(nchannels):
        for i in range(ndaq):
            tt = F(t[i * stride + c])
            if not (tt >= tmin and tt <= tmax):
                continue
            if not time_only:
                qq = F(q[i * stride + c])
                if not (qq >= qmin and qq <= qmax):
                    continue
                q1[c] = F(q1[c] + qq)
                q2[c] = F(q2[c] + F(qq * qq))
            m0[c] += 1
            t1[c] = F(t1[c] + tt)
            t2[c] = F(t2[c] + F(tt * tt))
    return m0, t1, t2, q1, q2


def moments_vec(t, q, nchannels, ndaq, stride, trange, qrange, time_only=True, state=None):
    tmin, tmax, qmin, qmax = F(trange[0]), F(trange[1]), F(qrange[0]), F(qrange[1])
    if state is None:
        state = (np.zeros(nchannels, np.uint32),) + tuple(np.zeros(nchannels, np.float32) for _ in range(4))
    m0, t1, t2, q1, q2 = (a.copy() for a in state)
    for i in range(ndaq):               # copies in order: float sums round as the device's do
        tt = _copy(np.asarray(t, np.float32), i, stride, nchannels)
        qq = _copy(np.asarray(q, np.float32), i, stride, nchannels)
        ok = (tt >= tmin) & (tt <= tmax)
        if not time_only:
            ok &= (qq >= qmin) & (qq <= qmax)
            q1[ok] += qq[ok]
            q2[ok] += qq[ok] * qq[ok]
        m0[ok] += 1
        t1[ok] += tt[ok]
        t2[ok] += tt[ok] * tt[ok]
    return m0, t1, t2, q1, q2


# ---- accumulate_kernel_eval (pdf.cu:267-368), in float64 --------------------------------------------------------
def kernel_eval_loop(event_hit, event_time, event_charge, t, q, nchannels, ndaq, stride, trange, qrange, inv_tbw, inv_qbw,
                     time_only=True, state=None):
    tmin, tmax, qmin, qmax = (float(F(x)) for x in (trange[0], trange[1], qrange[0], qrange[1]))
    if state is None:
        state = (np.zeros(nchannels, np.uint32), np.zeros(nchannels), np.zeros(nchannels))
    count, tv, qv = (a.copy() for a in state)

    def term(x, obs, ib, lo, hi, with_ib):
        arg = (x - obs) * ib
        norm = hi - lo
        if ib > 0:
            norm = (math.erf((hi - x) * ib / math.sqrt(2)) - math.erf((lo - x) * ib / math.sqrt(2))) * math.sqrt(math.pi / 2)
        return math.exp(-0.5 * arg * arg) * (ib if with_ib else 1.0) / norm

    for c in range(nchannels):
        for i in range(ndaq):
            tt = float(t[i * stride + c])
            if not (tt >= tmin and tt <= tmax):
                continue
            qq = float(q[i * stride + c])
            if not time_only and not (qq >= qmin and qq <= qmax):
                continue
            count[c] += 1
            if not event_hit[c]:
                continue
            tv[c] += term(tt, float(event_time[c]), float(inv_tbw[c]), tmin, tmax, time_only)
            if not time_only:
                qv[c] += term(qq, float(event_charge[c]), float(inv_qbw[c]), qmin, qmax, False)
    return count, tv, qv


def kernel_eval_vec(event_hit, event_time, event_charge, t, q, nchannels, ndaq, stride, trange, qrange, inv_tbw, inv_qbw,
                    time_only=True, state=None):
    tmin, tmax, qmin, qmax = (float(F(x)) for x in (trange[0], trange[1], qrange[0], qrange[1]))
    if state is None:
        state = (np.zeros(nchannels, np.uint32), np.zeros(nchannels), np.zeros(nchannels))
    count, tv, qv = (a.copy() for a in state)
    erf = np.vectorize(math.erf, otypes=[float])
    T = np.stack([_copy(np.asarray(t, np.float32), i, stride, nchannels) for i in range(ndaq)]).astype(float)
    Q = np.stack([_copy(np.asarray(q, np.float32), i, stride, nchannels) for i in range(ndaq)]).astype(float)
    ok = (T >= tmin) & (T <= tmax)
    if not time_only:
        ok &= (Q >= qmin) & (Q <= qmax)
    count += ok.sum(axis=0).astype(np.uint32)
    use = ok & np.asarray(event_hit).astype(bool)[None, :]

    def terms(X, obs, ib, lo, hi, with_ib):
        ib = np.asarray(ib, float)[None, :]
        arg = (X - np.asarray(obs, float)[None, :]) * ib
        with np.errstate(invalid='ignore', divide='ignore'):
            norm = np.where(ib > 0, (erf((hi - X) * ib / math.sqrt(2)) - erf((lo - X) * ib / math.sqrt(2))) * math.sqrt(math.pi / 2), hi - lo)
            v = np.exp(-0.5 * arg * arg) * (ib if with_ib else 1.0) / norm
        return np.where(use, v, 0.0).sum(axis=0)

    tv += terms(T, event_time, inv_tbw, tmin, tmax, time_only)
    if not time_only:
        qv += terms(Q, event_charge, inv_qbw, qmin, qmax, False)
    return count, tv, qv


# ---- random channel arrays ------------------------------------------------------------------------------------
def random_channels(rng, nchannels, ndaq, stride, trange=(0.0, 100.0), qmax=12.0, quantum=0.25):
    """MC channel arrays with sentinel times, ties (times on a grid), t just below tmax, negative charges."""
    n = ndaq * stride
    t = (np.round(rng.uniform(trange[0] - 10, trange[1] + 10, n) / quantum) * quantum).astype(np.float32)
    t[rng.random(n) < 0.3] = NOT_HIT
    t[rng.random(n) < 0.02] = np.nextafter(F(trange[1]), F(-np.inf))
    t[rng.random(n) < 0.02] = F(trange[1])
    t[rng.random(n) < 0.02] = F(trange[0])
    q = rng.uniform(-2, qmax, n).astype(np.float32)
    return t, q


def random_event(rng, nchannels, frac_hit=0.5, trange=(0.0, 100.0), quantum=0.25):
    hit = rng.random(nchannels) < frac_hit
    t = np.where(hit, np.round(rng.uniform(*trange, nchannels) / quantum) * quantum, 1e9).astype(np.float32)
    q = np.where(hit, rng.uniform(0, 10, nchannels), 0).astype(np.float32)
    return hit, t, q


@pytest.mark.parametrize('ndaq', [1, 3, 65])
def test_bin_hits_loop_equals_vectorised(ndaq):
    rng = np.random.default_rng(ndaq)
    nch, stride = 37, 40
    t, q = random_channels(rng, nch, ndaq, stride)
    a = bin_hits_loop(t, q, nch, ndaq, stride, 7, (0.0, 100.0), 3, (-0.5, 9.5))
    b = bin_hits_vec(t, q, nch, ndaq, stride, 7, (0.0, 100.0), 3, (-0.5, 9.5))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert a[0].sum() == a[1].sum() > 0
    assert np.array_equal(a[0], a[1].sum(axis=(1, 2)))


def test_bin_hits_clamps_and_truncates():
    # t just below tmax rounds up to bin tbins without the clamp; q = -1.5 counts as charge 0; q = 2.9 as 2
    tmin, tmax = F(-1.7), F(7.3)
    t = np.array([np.nextafter(tmax, F(0)), 1.0, 1.0], np.float32)
    q = np.array([0.5, -1.5, 2.9], np.float32)
    assert int((t[0] - tmin) / (tmax - tmin) * F(3)) == 3              # the reference's out-of-range bin
    hc, pdf = bin_hits_loop(t, q, 3, 1, 3, 3, (tmin, tmax), 4, (0.0, 4.0))
    assert np.array_equal(bin_hits_vec(t, q, 3, 1, 3, 3, (tmin, tmax), 4, (0.0, 4.0))[1], pdf)
    assert hc.tolist() == [1, 1, 1]
    assert pdf[0, 2, 0] == 1 and pdf[1, 0, 0] == 1 and pdf[2, 0, 2] == 1


@pytest.mark.parametrize('ndaq,k', [(1, 1), (64, 5), (130, 40)])
def test_eval_accumulate_loop_equals_vectorised(ndaq, k):
    rng = np.random.default_rng(10 + ndaq)
    nch, stride = 23, 25
    hit, et, _ = random_event(rng, nch)
    t, _ = random_channels(rng, nch, ndaq, stride)
    state_a = state_b = None
    for _ in range(3):             # carry-over between calls
        state_a = eval_accumulate_loop(hit, et, t, nch, ndaq, stride, 2.0, (0.0, 100.0), k, state_a)
        state_b = eval_accumulate_vec(hit, et, t, nch, ndaq, stride, 2.0, (0.0, 100.0), k, state_b)
    for x, y in zip(state_a, state_b):
        assert np.array_equal(x, y)
    assert (state_a[2] < 1e9).any()


def test_eval_accumulate_carry_over_equals_one_call():
    rng = np.random.default_rng(3)
    nch, ndaq = 19, 128
    hit, et, _ = random_event(rng, nch)
    t, _ = random_channels(rng, nch, ndaq, nch)
    one = eval_accumulate_vec(hit, et, t, nch, ndaq, nch, 2.0, (0.0, 100.0), 7)
    state = None
    for i in range(ndaq):
        state = eval_accumulate_loop(hit, et, t[i * nch:(i + 1) * nch], nch, 1, nch, 2.0, (0.0, 100.0), 7, state)
    for x, y in zip(one, state):
        assert np.array_equal(x, y)


@pytest.mark.parametrize('time_only', [True, False])
def test_moments_and_kernel_loop_equal_vectorised(time_only):
    rng = np.random.default_rng(4)
    nch, ndaq, stride = 17, 9, 20
    hit, et, eq = random_event(rng, nch)
    t, q = random_channels(rng, nch, ndaq, stride)
    a = moments_loop(t, q, nch, ndaq, stride, (0.0, 100.0), (0.0, 10.0), time_only)
    b = moments_vec(t, q, nch, ndaq, stride, (0.0, 100.0), (0.0, 10.0), time_only)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    itb = rng.uniform(0, 1, nch).astype(np.float32)
    itb[::4] = 0
    iqb = rng.uniform(0, 2, nch).astype(np.float32)
    a = kernel_eval_loop(hit, et, eq, t, q, nch, ndaq, stride, (0.0, 100.0), (0.0, 10.0), itb, iqb, time_only)
    b = kernel_eval_vec(hit, et, eq, t, q, nch, ndaq, stride, (0.0, 100.0), (0.0, 10.0), itb, iqb, time_only)
    assert np.array_equal(a[0], b[0])
    assert np.allclose(a[1], b[1], rtol=1e-12, atol=0) and np.allclose(a[2], b[2], rtol=1e-12, atol=0)
    assert (a[1] > 0).any()


# ---- host arithmetic -------------------------------------------------------------------------------------------
def test_pdf_eval_values_high_and_low_stats():
    from chroma_amd.gpu.pdf import pdf_eval_values
    k = 4
    hit = np.array([1, 1, 1, 0, 1], bool)
    hitcount = np.array([50, 20, 10, 30, 0], np.uint32)
    bincount = np.array([8, 2, 0, 0, 0], np.uint32)
    nearest = np.full((5, k), 1e9, np.float32)
    nearest[1] = [0.1, 0.2, 0.4, 1e9]                 # low stats: 3 distances
    nearest[2] = [1e9] * k                           # low stats, nothing found: first entry
    value, uncert = pdf_eval_values(hit, hitcount, bincount, nearest, 0.5, k)
    assert value[0] == pytest.approx(8 / 50 / 0.5) and uncert[0] == pytest.approx(value[0] / np.sqrt(8))
    assert value[1] == pytest.approx(3 / 20 / np.float32(0.4) / 2) and uncert[1] == pytest.approx(value[1] / np.sqrt(3))
    assert value[2] == pytest.approx(1 / 10 / 1e9 / 2)
    assert value[3] == 0 and value[4] == 0           # not hit in the event / no MC


def test_kernel_bandwidths_formula():
    from chroma_amd.gpu.pdf import kernel_bandwidths
    hitcount = np.array([100, 0, 4], np.uint32)
    tmom1 = np.array([100 * 5.0, 0, 4 * 2.0], np.float32)
    tmom2 = np.array([100 * (25.0 + 4.0), 0, 4 * 4.0], np.float32)       # rms 2, and rms 0
    event_time = np.array([6.0, 0.0, 2.0])
    inv_t, inv_q = kernel_bandwidths(hitcount, tmom1, tmom2, event_time, True, scale_factor=2.0)
    factor = ((4.0 / 3) / (100 / 2.0)) ** (-1.0 / 5)
    density = min(1 / 2.0, np.exp(-0.5 * (1.0 / 2.0)) / np.sqrt(2 * np.pi) / 2.0)
    assert inv_t[0] == pytest.approx(density / factor, rel=1e-6)
    assert inv_t[1] == 0 and inv_t[2] == 0                              # no spread: no bandwidth
    assert inv_t.dtype == np.float32 and not inv_q.any()
    inv_t2, inv_q2 = kernel_bandwidths(hitcount[:1], tmom1[:1], tmom2[:1], event_time[:1], False,
                                       np.array([300.0], np.float32), np.array([1000.0], np.float32), np.array([3.0]))
    factor2 = ((4.0 / 4) / 100) ** (-1.0 / 6)
    assert inv_q2[0] == pytest.approx(min(1.0, np.exp(0.0) / np.sqrt(2 * np.pi)) / factor2, rel=1e-6)


# ---- Likelihood NLL composition ---------------------------------------------------------------------------------
class _StubSim(object):
    def __init__(self, hitcount, pdf):
        self.hitcount, self.pdf = hitcount, pdf
        self.calls = []

    def eval_pdf(self, channels, iterable, min_twidth, trange, min_qwidth, qrange, **kw):
        self.calls.append((list(iterable), min_twidth, kw))
        return self.hitcount.copy(), self.pdf.copy(), self.pdf * 0.1


def test_likelihood_nll_composition():
    from chroma_amd.event import Channels, Event
    from chroma_amd.likelihood import Likelihood
    hit = np.array([True, True, False, False, True])
    ev = Event()
    ev.channels = Channels(hit, np.zeros(5, np.float32), np.zeros(5, np.float32))
    nevals, nreps, ndaq = 2, 3, 5
    ntotal = nevals * nreps * ndaq
    hitcount = np.array([15, 0, 30, 3, 6], np.uint32)
    pdf = np.array([0.02, 0.0, 0.5, 0.1, np.nan])
    sim = _StubSim(hitcount, pdf)
    like = Likelihood(sim, ev, trange=(-0.5, 999.5))
    nll = like.eval(iter(range(100)), nevals, nreps=nreps, ndaq=ndaq)
    p = hitcount / ntotal
    p = np.where(hit, p, 1 - p)
    p = np.maximum(p, 0.5 / ntotal)                   # channel 1: never hit in the MC; channel 2: always hit, not in data
    floor = 1.0 / 1000.0                              # PDF floor for the zero and NaN densities
    want = -(np.log(p).sum() + np.log([0.02, floor, floor]).sum())
    assert nll.nominal_value == pytest.approx(want, rel=1e-6) and nll.std_dev == 0
    assert nll.nominal_value > 0                      # a negative LOG likelihood of probabilities < 1
    assert sim.calls[0][0] == [0, 1] and sim.calls[0][1] == 0.2 and sim.calls[0][2]['min_bin_content'] == 320


def test_measurement_arithmetic():
    from chroma_amd.likelihood import Measurement
    m = -(Measurement(1.0, 3.0) + Measurement(2.0, 4.0))
    assert m.nominal_value == -3.0 and m.std_dev == 5.0 and m < 0


def test_the_chroma_alias_resolves_the_pdf_layer():
    import importlib
    import chroma
    likelihood = importlib.import_module('chroma.likelihood')
    from chroma_amd import likelihood as real
    assert likelihood is real and hasattr(likelihood, 'Likelihood')
    from chroma import gpu
    from chroma_amd.gpu.pdf import GPUPDF, GPUKernelPDF
    assert gpu.GPUPDF is GPUPDF and gpu.GPUKernelPDF is GPUKernelPDF
    from chroma.sim import Simulation
    for name in ('create_pdf', 'eval_pdf', 'setup_kernel', 'eval_kernel'):
        assert callable(getattr(Simulation, name))
    assert chroma is not None
