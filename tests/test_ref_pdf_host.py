"""The NumPy restatements of tests/test_pdf_host.py against the reference's OWN PDF kernels (chroma/cuda/pdf.cu with
sorting.h, compiled for the host by oracle/ref_pdf_driver.cc into oracle/_ref/libchroma_ref_pdf.so).  No GPU.

Both forms of every restatement (`*_loop` and `*_vec`) are held to the library on inputs for which the reference is
defined: charges in [0, 2^32), no time whose unclamped bin index equals tbins (asserted: none occurs), no NaN, and
k + ndaq <= 1000 (the reference's distance table).  Counts and histograms: exact.  Nearest-distance tables and moments:
bit for bit.  Kernel sums are float32 in the reference and float64 in the restatement:

    the largest relative difference over KERNEL_CASES, three carried calls each, measured here on the CPU against the
    host libm, is 8.2e-6 (REF_KERNEL_F32_ERROR below is that figure rounded up; the test asserts it is not exceeded).

tests/test_gpu_pdf_edges.py runs the device on the same KERNEL_CASES and takes its tolerance from that figure.

Result: the restatements and the reference agree everywhere in their common domain; no new deviation was found.  The
deviations that remain are the ones DESIGN.md lists: clamped bins, every copy binned, and NaN as "not hit"."""
import numpy as np
import pytest

import oracle
from test_pdf_host import (F, NOT_HIT, bin_hits_loop, bin_hits_vec, eval_accumulate_loop, eval_accumulate_vec,
                           kernel_eval_loop, kernel_eval_vec, moments_loop, moments_vec)

pytestmark = pytest.mark.skipif(not oracle.have_ref_pdf(), reason='oracle/_ref/libchroma_ref_pdf.so is not built')

TRANGE, QRANGE = (0.0, 100.0), (0.0, 10.0)
REF_KERNEL_F32_ERROR = 8.3e-6        # see the module docstring: float32 reference sums against the float64 restatement
KERNEL_ATOL = 1e-30                 # sums whose every term underflows: a float32 term below FLT_MIN = 1.2e-38 has no
                                    # relative precision left, and the norms that divide it are above 1e-3 here


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def mc_channels(rng, nch, ndaq, stride, event_time=None, near=None, offgrid=0.3):
    """MC channel arrays inside the reference's domain: times on a 0.25 grid (ties) and off it, the 1e9 sentinel, t
    exactly tmin and exactly tmax, charges in [0, 12) with some exactly on QRANGE's ends.  The padding [nch, stride) holds
    in-window values that no kernel may count.  ``near`` (per channel, with ``event_time``): the fraction of copies put
    within 0.75 of the event's time, so that some channels fill their minimum bin and some never do."""
    n = ndaq * stride
    t = np.round(rng.uniform(TRANGE[0] - 10, TRANGE[1] + 10, n) * 4) / 4
    off = rng.random(n) < offgrid
    t[off] = rng.uniform(TRANGE[0] - 10, TRANGE[1] + 10, off.sum())
    t = t.astype(np.float32).reshape(ndaq, stride)
    if near is not None:
        close = rng.random((ndaq, nch)) < np.asarray(near)[None, :]
        t[:, :nch] = np.where(close, np.asarray(event_time, np.float32)[None, :] + rng.integers(-3, 4, (ndaq, nch)) * F(0.25),
                              t[:, :nch])
    t[rng.random((ndaq, stride)) < 0.25] = NOT_HIT
    t[rng.random((ndaq, stride)) < 0.03] = F(TRANGE[0])
    t[rng.random((ndaq, stride)) < 0.03] = F(TRANGE[1])
    q = rng.uniform(0, 12, (ndaq, stride)).astype(np.float32)
    q[rng.random((ndaq, stride)) < 0.03] = F(QRANGE[0])
    q[rng.random((ndaq, stride)) < 0.03] = F(QRANGE[1])
    t[:, nch:] = 50.0
    q[:, nch:] = 5.0
    return t.reshape(-1), q.reshape(-1)


def mc_event(rng, nch, frac_hit=0.6):
    hit = rng.random(nch) < frac_hit
    t = np.where(hit, np.round(rng.uniform(5, 95, nch) * 4) / 4, 1e9).astype(np.float32)
    q = np.where(hit, rng.uniform(0, 10, nch), 0).astype(np.float32)
    return hit, t, q


def unclamped_bins(x, lo, hi, bins):
    x = np.asarray(x, np.float32)
    return ((x - F(lo)) / (F(hi) - F(lo)) * F(bins)).astype(np.int64)


# ---- bin_hits ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ndaq,tbins,qbins', [(1, 8, 5), (3, 1, 1), (65, 16, 10)])
def test_bin_hits_is_the_reference(ndaq, tbins, qbins):
    rng = np.random.default_rng(300 + ndaq)
    nch, stride = 37, 40
    t, q = mc_channels(rng, nch, ndaq, stride, offgrid=0.0)          # the grid keeps every time's bin below tbins
    t[:2] = TRANGE
    q[::11] = F(4294967040.0)                 # the largest float below 2^32: outside the charge range, inside the domain
    qrange = (-0.5, 9.5)
    inside = (t >= F(TRANGE[0])) & (t < F(TRANGE[1]))
    assert (t[inside] == F(TRANGE[0])).any() and (t == F(TRANGE[1])).any()
    # the reference's domain: no in-range time or charge whose unclamped bin is `bins` (it would land in the next row)
    assert (unclamped_bins(t[inside], *TRANGE, tbins) == tbins).sum() == 0
    qq = np.floor(q).astype(np.float32)
    assert (unclamped_bins(qq[(qq >= F(qrange[0])) & (qq < F(qrange[1]))], *qrange, qbins) == qbins).sum() == 0
    want = got_l = got_v = None
    for _ in range(3):
        want = oracle.ref_bin_hits(t, q, nch, ndaq, stride, tbins, TRANGE, qbins, qrange, *(want or ()))
        got_l = bin_hits_loop(t, q, nch, ndaq, stride, tbins, TRANGE, qbins, qrange, *(got_l or ()))
        got_v = bin_hits_vec(t, q, nch, ndaq, stride, tbins, TRANGE, qbins, qrange, *(got_v or ()))
    for got in (got_l, got_v):
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert got_l[0].sum() > 0 and np.array_equal(got_l[0], got_l[1].sum(axis=(1, 2)))
    # tmax itself is outside (bin_hits is exclusive there), tmin inside
    only = np.array([TRANGE[0], TRANGE[1]], np.float32)
    hc, _ = oracle.ref_bin_hits(only, np.ones(2, np.float32), 2, 1, 2, tbins, TRANGE, qbins, qrange)
    assert hc.tolist() == [1, 0] and bin_hits_vec(only, np.ones(2, np.float32), 2, 1, 2, tbins, TRANGE, qbins, qrange)[0].tolist() == [1, 0]


# ---- accumulate_bincount + accumulate_nearest_neighbor ----------------------------------------------------------
EVAL_CASES = [(1, 1), (1, 2), (3, 64), (64, 5), (65, 100), (130, 40), (63, 129), (200, 37), (64, 320), (1, 999), (200, 800)]


@pytest.mark.parametrize('ndaq,k', EVAL_CASES)
def test_eval_accumulate_is_the_reference(ndaq, k):
    rng = np.random.default_rng(1000 * ndaq + k)
    nch, stride = 23, 26
    hit, et, _ = mc_event(rng, nch)
    hit[:2] = [True, False]
    et[0] = 50.0
    near = np.linspace(0.0, 1.0, nch)             # channel 0 never fills its minimum bin; the last ones soon do
    near[-1] = 1.0
    hit[-1], et[-1] = True, 40.0
    ref = loop = vec = None
    for _ in range(3):                             # three carried calls
        t, _ = mc_channels(rng, nch, ndaq, stride, et, near)
        t[0::stride] = NOT_HIT                     # channel 0: one MC hit per call, outside its minimum bin
        t[0] = et[0] + F(7.25)
        ref = oracle.ref_eval_accumulate(hit, et, t, nch, ndaq, stride, 2.0, TRANGE, k, ref)
        loop = eval_accumulate_loop(hit, et, t, nch, ndaq, stride, 2.0, TRANGE, k, loop)
        vec = eval_accumulate_vec(hit, et, t, nch, ndaq, stride, 2.0, TRANGE, k, vec)
    for got in (loop, vec):
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
        assert np.array_equal(bits(got[2]), bits(ref[2]))
    # floors, on the restatement alone
    hitcount, bincount, nearest = loop
    filled = (nearest < 1e8).sum(axis=1)
    assert hitcount[hit].any() and hitcount[~hit].any() and not bincount[~hit].any()
    assert (bincount[hit] < k).any()
    if 3 * ndaq >= 2 * k:                          # enough copies for the channel that is always near its event time
        assert (bincount[hit] >= k).any()
    if k > 3:
        assert filled[0] == 3                      # a partly filled table
    assert (nearest[hit] < 1e8).any() and (nearest[~hit] == NOT_HIT).all()


def test_eval_accumulate_wrapper_refuses_what_the_reference_table_cannot_hold():
    hit, et = np.ones(2, bool), np.full(2, 50.0, np.float32)
    t = np.full(2 * 2, 50.0, np.float32)
    with pytest.raises(ValueError):
        oracle.ref_eval_accumulate(hit, et, t, 2, 2, 2, 2.0, TRANGE, 999)
    lib = oracle.load_ref_pdf()
    assert lib.ref_pdf_eval_accumulate(2, 2, None, None, None, None, None, 2.0, 0.0, 100.0, 999, 2, None, None, None) == -2
    assert oracle.ref_eval_accumulate(hit, et, t, 2, 2, 2, 2.0, TRANGE, 998)[1].tolist() == [2, 2]


def test_eval_accumulate_no_hit_channel():
    rng = np.random.default_rng(5)
    nch, ndaq = 9, 4
    hit, et = np.zeros(nch, bool), np.full(nch, 1e9, np.float32)
    t, _ = mc_channels(rng, nch, ndaq, nch)
    ref = oracle.ref_eval_accumulate(hit, et, t, nch, ndaq, nch, 2.0, TRANGE, 3)
    got = eval_accumulate_vec(hit, et, t, nch, ndaq, nch, 2.0, TRANGE, 3)
    for a, b in zip(got, ref):
        assert np.array_equal(a, b)
    assert got[0].any() and not got[1].any()


# ---- accumulate_moments -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('time_only', [True, False])
@pytest.mark.parametrize('ndaq', [1, 9, 65])
def test_moments_are_the_reference(time_only, ndaq):
    rng = np.random.default_rng(40 + ndaq)
    nch, stride = 29, 32
    ref = loop = vec = None
    for _ in range(3):
        t, q = mc_channels(rng, nch, ndaq, stride)
        ref = oracle.ref_moments(t, q, nch, ndaq, stride, TRANGE, QRANGE, time_only, ref)
        loop = moments_loop(t, q, nch, ndaq, stride, TRANGE, QRANGE, time_only, loop)
        vec = moments_vec(t, q, nch, ndaq, stride, TRANGE, QRANGE, time_only, vec)
    for got in (loop, vec):
        assert np.array_equal(got[0], ref[0])
        for a, b in zip(got[1:], ref[1:]):
            assert np.array_equal(bits(a), bits(b))
    assert loop[0].any() and loop[1].any() and (time_only or loop[3].any())
    # both window ends are inside (inclusive at tmax and qmax, unlike bin_hits)
    ends_t = np.array([TRANGE[0], TRANGE[1], TRANGE[1]], np.float32)
    ends_q = np.array([QRANGE[0], QRANGE[1], 5.0], np.float32)
    assert oracle.ref_moments(ends_t, ends_q, 3, 1, 3, TRANGE, QRANGE, time_only)[0].tolist() == [1, 1, 1]
    assert moments_vec(ends_t, ends_q, 3, 1, 3, TRANGE, QRANGE, time_only)[0].tolist() == [1, 1, 1]


# ---- accumulate_kernel_eval ---------------------------------------------------------------------------------------
# (nchannels, ndaq, time_only): also the one-thread-per-channel sizes of tests/test_gpu_pdf_edges.py
KERNEL_CASES = [(1, 1, True), (1, 65, False), (67, 2, True), (67, 2, False), (255, 2, False), (256, 65, True), (257, 65, False),
                (513, 1, True), (513, 2, False)]
BANDWIDTHS = (0.0, 1e-4, 1.0, 1e3)         # flat kernel, wider than the window, of the grid's order, far narrower


def kernel_case(nch, ndaq, time_only, call=0):
    """One call's inputs of a KERNEL_CASES entry: the event (fixed over the calls) and that call's MC.  Every inverse
    bandwidth of BANDWIDTHS (and a random one) meets every channel kind; times and charges sit on both window ends."""
    rng = np.random.default_rng(7000 + 10 * nch + ndaq + 2 * time_only)
    stride = nch + 3
    hit, et, eq = mc_event(rng, nch, 0.7)
    if nch == 1:
        hit[:] = True
        et[:] = 50.0
    c = np.arange(nch)
    itb = np.array(BANDWIDTHS + (0.0,), np.float32)[c % 5]
    itb[c % 5 == 4] = rng.uniform(0.02, 2.0, (c % 5 == 4).sum())
    iqb = np.array(BANDWIDTHS[::-1] + (0.0,), np.float32)[(c // 5) % 5]
    iqb[(c // 5) % 5 == 4] = rng.uniform(0.1, 2.0, ((c // 5) % 5 == 4).sum())
    if nch == 1:
        itb[:], iqb[:] = 1.0, 1e3
    for _ in range(call + 1):
        t, q = mc_channels(rng, nch, ndaq, stride, et, np.full(nch, 0.4))
        if nch >= 4:                       # both ends of both windows, in every call
            t[:4] = [TRANGE[0], TRANGE[1], 50.0, 50.0]
            q[:4] = [5.0, 5.0, QRANGE[0], QRANGE[1]]
    return dict(hit=hit, et=et, eq=eq, t=t, q=q, nch=nch, ndaq=ndaq, stride=stride, itb=itb, iqb=iqb, time_only=time_only)


def kernel_args(case):
    return (case['hit'], case['et'], case['eq'], case['t'], case['q'], case['nch'], case['ndaq'], case['stride'], TRANGE, QRANGE,
            case['itb'], case['iqb'], case['time_only'])


def relative_error(got, want, atol=KERNEL_ATOL):
    """Largest |got - want| / |want| over the entries the absolute floor does not already pass."""
    got, want = np.asarray(got, float), np.asarray(want, float)
    err = np.abs(got - want)
    judged = err > atol
    assert np.isfinite(got).all() and np.isfinite(want).all() and (want[judged] != 0).all()
    return float((err[judged] / np.abs(want[judged])).max()) if judged.any() else 0.0


_kernel_reference = {}


def kernel_reference(i, ncalls=3):
    """(count, time sums, charge sums) in float64 after each of ``ncalls`` carried calls of KERNEL_CASES[i]: computed once
    (the vectorised restatement), shared by the tests here and on the device, and never written to."""
    if i not in _kernel_reference:
        out, state = [], None
        for call in range(ncalls):
            state = kernel_eval_vec(*kernel_args(kernel_case(*KERNEL_CASES[i], call=call)), state=state)
            for a in state:
                a.setflags(write=False)
            out.append(state)
        _kernel_reference[i] = out
    return _kernel_reference[i]


@pytest.mark.parametrize('i', range(len(KERNEL_CASES)))
def test_kernel_eval_is_the_reference(i):
    nch, ndaq, time_only = KERNEL_CASES[i]
    ref = loop = None
    worst = 0.0
    for call, vec in enumerate(kernel_reference(i)):
        case = kernel_case(nch, ndaq, time_only, call)
        inside = (case['t'] >= F(TRANGE[0])) & (case['t'] <= F(TRANGE[1]))
        if nch > 1:
            assert (case['t'] == F(TRANGE[0])).any() and (case['t'] == F(TRANGE[1])).any()
            assert (case['q'][inside] == F(QRANGE[0])).any() and (case['q'][inside] == F(QRANGE[1])).any()
        ref = oracle.ref_kernel_eval(*kernel_args(case), state=ref)
        if nch <= 67:                      # the per-channel loop, where it is quick
            loop = kernel_eval_loop(*kernel_args(case), state=loop)
            assert np.array_equal(loop[0], vec[0])
            assert np.allclose(loop[1], vec[1], rtol=1e-12, atol=0) and np.allclose(loop[2], vec[2], rtol=1e-12, atol=0)
        assert np.array_equal(ref[0], vec[0])
        worst = max(worst, relative_error(ref[1], vec[1]), relative_error(ref[2], vec[2]))
    print('kernel_eval case %d %r: float32 reference against float64, largest relative difference %.3g' % (i, KERNEL_CASES[i], worst))
    assert worst <= REF_KERNEL_F32_ERROR
    count, tv, qv = kernel_reference(i)[-1]
    assert count.any() and (tv > KERNEL_ATOL).any() and (time_only or (qv > KERNEL_ATOL).any())
    if nch > 5:
        hit = kernel_case(nch, ndaq, time_only)['hit']
        assert not tv[~hit].any() and count[~hit].any()
