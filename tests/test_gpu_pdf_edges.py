"""The PDF kernels (chroma_amd/csrc/kernels_pdf.h) at their size edges, through the C entry points, with guard words
behind every output.  Comparands: the NumPy restatements of tests/test_pdf_host.py and, where its domain allows and the
library is built, the reference's own pdf.cu (oracle/_ref/libchroma_ref_pdf.so, see tests/test_ref_pdf_host.py).

Histograms, counts and nearest-distance tables: exact (tables bit for bit).  Moments: bit for bit.  Kernel sums against
float64: relative KERNEL_RTOL = max(1e-5, 4 * REF_KERNEL_F32_ERROR) = 3.32e-5 -- the project's 1e-5, or four times the
8.3e-6 that the reference's own float32 sums (host libm) differ from float64 on the same KERNEL_CASES, whichever is
larger; the factor covers the device's expf / erff differing from libm's by a few ulp per term.  Sums below
KERNEL_ATOL = 1e-30 (every term underflowed) pass on the absolute floor."""
import numpy as np
import pytest

import oracle
from test_pdf_host import (F, NOT_HIT, bin_hits_loop, bin_hits_vec, eval_accumulate_loop, eval_accumulate_vec,
                           kernel_eval_vec, moments_vec)
from test_ref_pdf_host import (KERNEL_ATOL, KERNEL_CASES, QRANGE, REF_KERNEL_F32_ERROR, TRANGE, bits, kernel_args,
                               kernel_case, kernel_reference, mc_channels, mc_event, unclamped_bins)

pytestmark = pytest.mark.gpu

KERNEL_RTOL = max(1e-5, 4 * REF_KERNEL_F32_ERROR)
NGUARD, GUARD = 64, 0xDEADBEEF
ROW_SENTINEL = F(-777.0)                # what the nearest rows of unlisted hits hold
HAVE_REF = oracle.have_ref_pdf()


@pytest.fixture(scope='module')
def gpu():
    from chroma_amd import gpu as g
    ctx = g.create_cuda_context(0)
    yield g
    ctx.pop()


class Guarded(object):
    """A device copy of a host array with NGUARD sentinel words behind it; ``get`` asserts they are still there."""

    def __init__(self, gpu, host):
        host = np.ascontiguousarray(host)
        assert host.dtype.itemsize == 4
        self.dtype, self.n = host.dtype, host.size
        self.dev = gpu.to_gpu(np.concatenate([host.reshape(-1).view(np.uint32), np.full(NGUARD, GUARD, np.uint32)]))
        self.ptr = self.dev.ptr

    def get(self):
        words = self.dev.get()
        assert (words[self.n:] == GUARD).all(), 'guard words behind an output were overwritten'
        return words[:self.n].view(self.dtype).copy()


def _call(gpu, name, *args):
    from chroma_amd import _lib
    ctx = gpu.get_context()
    _lib.check(getattr(ctx._lib, name)(ctx.handle, *args))


def dev_bin_hits(gpu, t, q, nch, ndaq, stride, tbins, trange, qbins, qrange, hitcount=None, pdf=None):
    hc = Guarded(gpu, np.zeros(nch, np.uint32) if hitcount is None else hitcount)
    hist = Guarded(gpu, np.zeros(nch * tbins * qbins, np.uint32) if pdf is None else pdf)
    dt, dq = gpu.to_gpu(np.asarray(t, np.float32)), gpu.to_gpu(np.asarray(q, np.float32))
    _call(gpu, 'chroma_pdf_bin_hits', nch, ndaq, stride, dq.ptr, dt.ptr, tbins, float(trange[0]), float(trange[1]), qbins,
          float(qrange[0]), float(qrange[1]), hc.ptr, hist.ptr)
    return hc.get(), hist.get().reshape(nch, tbins, qbins)


def dev_eval_raw(gpu, event_hit, et, t, nch, ndaq, stride, min_twidth, trange, k, hit_list, hitcount, bincount, rows):
    """chroma_pdf_eval_accumulate on a caller's hit list and hit-indexed table ``rows`` [>= len(hit_list)][k]."""
    hc, bc, tab = Guarded(gpu, hitcount), Guarded(gpu, bincount), Guarded(gpu, np.asarray(rows, np.float32))
    d_hit = gpu.to_gpu(np.asarray(event_hit).astype(np.uint32))
    d_et, d_t = gpu.to_gpu(np.asarray(et, np.float32)), gpu.to_gpu(np.asarray(t, np.float32))
    d_list = gpu.to_gpu(np.concatenate([np.asarray(hit_list, np.uint32), np.zeros(1, np.uint32)]))
    _call(gpu, 'chroma_pdf_eval_accumulate', nch, ndaq, stride, d_hit.ptr, d_et.ptr, d_t.ptr, len(hit_list), d_list.ptr,
          float(min_twidth), float(trange[0]), float(trange[1]), k, hc.ptr, bc.ptr, tab.ptr)
    return hc.get(), bc.get(), tab.get().reshape(np.shape(rows))


def dev_eval(gpu, event_hit, et, t, nch, ndaq, stride, min_twidth, trange, k, state=None):
    """The argument list and the (hitcount, bincount, nearest[nch, k]) state of the restatements.  The hit-indexed table
    carries two more rows than hits, filled with ROW_SENTINEL, which have to stay."""
    hit = np.asarray(event_hit).astype(bool)
    if state is None:
        state = (np.zeros(nch, np.uint32), np.zeros(nch, np.uint32), np.full((nch, k), NOT_HIT, np.float32))
    hit_list = np.flatnonzero(hit)
    rows = np.full((len(hit_list) + 2, k), ROW_SENTINEL, np.float32)
    rows[:len(hit_list)] = state[2][hit_list]
    hc, bc, rows = dev_eval_raw(gpu, hit, et, t, nch, ndaq, stride, min_twidth, trange, k, hit_list, state[0], state[1], rows)
    assert (rows[len(hit_list):] == ROW_SENTINEL).all()
    nearest = state[2].copy()
    nearest[hit_list] = rows[:len(hit_list)]
    return hc, bc, nearest


def dev_moments(gpu, t, q, nch, ndaq, stride, trange, qrange, time_only=True, state=None):
    if state is None:
        state = (np.zeros(nch, np.uint32),) + tuple(np.zeros(nch, np.float32) for _ in range(4))
    out = [Guarded(gpu, a) for a in state]
    dt, dq = gpu.to_gpu(np.asarray(t, np.float32)), gpu.to_gpu(np.asarray(q, np.float32))
    _call(gpu, 'chroma_pdf_moments', int(time_only), nch, ndaq, stride, dt.ptr, dq.ptr, float(trange[0]), float(trange[1]),
          float(qrange[0]), float(qrange[1]), *[a.ptr for a in out])
    return tuple(a.get() for a in out)


def dev_kernel_eval(gpu, event_hit, et, eq, t, q, nch, ndaq, stride, trange, qrange, itb, iqb, time_only=True, state=None):
    """State and result: (hitcount, float32 time sums, float32 charge sums)."""
    if state is None:
        state = (np.zeros(nch, np.uint32), np.zeros(nch, np.float32), np.zeros(nch, np.float32))
    out = [Guarded(gpu, a) for a in state]
    ins = [gpu.to_gpu(np.asarray(a, np.float32)) for a in (et, eq, t, q, itb, iqb)]
    d_hit = gpu.to_gpu(np.asarray(event_hit).astype(np.uint32))
    _call(gpu, 'chroma_pdf_kernel_eval', int(time_only), nch, ndaq, stride, d_hit.ptr, ins[0].ptr, ins[1].ptr, ins[2].ptr,
          ins[3].ptr, float(trange[0]), float(trange[1]), float(qrange[0]), float(qrange[1]), ins[4].ptr, ins[5].ptr,
          *[a.ptr for a in out])
    return tuple(a.get() for a in out)


def same_state(got, want):
    """Counts exact, float arrays bit for bit."""
    assert len(got) == len(want)
    for a, b in zip(got, want):
        if np.asarray(b).dtype == np.float32:
            assert np.array_equal(bits(a), bits(b))
        else:
            assert np.array_equal(a, b)


def close_sums(got, want):
    got, want = np.asarray(got, float), np.asarray(want, float)
    err = np.abs(got - want)
    bad = ~(err <= KERNEL_RTOL * np.abs(want) + KERNEL_ATOL)
    assert not bad.any(), (np.flatnonzero(bad)[:8], got[bad][:8], want[bad][:8])


# ---- one thread per channel: bin_hits, eval_hitcount, moments, kernel_eval (hit counts) ------------------------------
@pytest.mark.parametrize('ndaq', [1, 2, 65])
@pytest.mark.parametrize('nch', [1, 255, 256, 257, 513])
def test_one_thread_per_channel(gpu, nch, ndaq):
    rng = np.random.default_rng(17 * nch + ndaq)
    stride = nch + 5                              # the padding holds in-window times and charges: never counted
    hit, et, eq = mc_event(rng, nch, 0.5)
    itb = rng.uniform(0.02, 2.0, nch).astype(np.float32)
    tbins, qbins, qrange_bins, k = 8, 5, (-0.5, 9.5), 5
    got_bins = got_eval = want_bins = want_eval = ref_bins = ref_eval = None
    got_mom, want_mom, ref_mom = [None, None], [None, None], [None, None]
    got_kern, want_kern = [None, None], [None, None]
    for call in range(2):
        t, q = mc_channels(rng, nch, ndaq, stride, offgrid=0.0)            # on the grid: no bin index rounds up to tbins
        inside = (t >= F(TRANGE[0])) & (t < F(TRANGE[1]))
        assert (unclamped_bins(t[inside], *TRANGE, tbins) == tbins).sum() == 0
        got_bins = dev_bin_hits(gpu, t, q, nch, ndaq, stride, tbins, TRANGE, qbins, qrange_bins, *(got_bins or ()))
        want_bins = bin_hits_vec(t, q, nch, ndaq, stride, tbins, TRANGE, qbins, qrange_bins, *(want_bins or ()))
        got_eval = dev_eval(gpu, hit, et, t, nch, ndaq, stride, 2.0, TRANGE, k, got_eval)
        want_eval = eval_accumulate_vec(hit, et, t, nch, ndaq, stride, 2.0, TRANGE, k, want_eval)
        if HAVE_REF:
            ref_bins = oracle.ref_bin_hits(t, q, nch, ndaq, stride, tbins, TRANGE, qbins, qrange_bins, *(ref_bins or ()))
            ref_eval = oracle.ref_eval_accumulate(hit, et, t, nch, ndaq, stride, 2.0, TRANGE, k, ref_eval)
        for m, time_only in enumerate((True, False)):
            got_mom[m] = dev_moments(gpu, t, q, nch, ndaq, stride, TRANGE, QRANGE, time_only, got_mom[m])
            want_mom[m] = moments_vec(t, q, nch, ndaq, stride, TRANGE, QRANGE, time_only, want_mom[m])
            if HAVE_REF:
                ref_mom[m] = oracle.ref_moments(t, q, nch, ndaq, stride, TRANGE, QRANGE, time_only, ref_mom[m])
            got_kern[m] = dev_kernel_eval(gpu, hit, et, eq, t, q, nch, ndaq, stride, TRANGE, QRANGE, itb, itb, time_only, got_kern[m])
            want_kern[m] = kernel_eval_vec(hit, et, eq, t, q, nch, ndaq, stride, TRANGE, QRANGE, itb, itb, time_only, want_kern[m])
    same_state(got_bins, want_bins)
    same_state(got_eval, want_eval)
    assert want_bins[0].sum() == want_bins[1].sum() and (nch == 1 or (want_eval[0][~hit].any() and want_eval[0][hit].any()))
    for m in range(2):
        same_state(got_mom[m], want_mom[m])
        assert np.array_equal(got_kern[m][0], want_kern[m][0])
        assert not got_kern[m][1][~hit].any() and not got_kern[m][2][~hit].any()
        assert nch == 1 or want_kern[m][0].any()
    assert not got_mom[0][3].any() and not got_mom[0][4].any() and not got_kern[0][2].any()         # time only: charge arrays untouched
    if HAVE_REF:
        same_state(got_bins, ref_bins)
        same_state(got_eval, ref_eval)
        for m in range(2):
            same_state(got_mom[m], ref_mom[m])


# ---- bin_hits: window ends, charge conversion, clamps, refusals -----------------------------------------------------
def test_bin_hits_edges(gpu):
    tmin, tmax = F(-1.7), F(7.3)
    below = np.nextafter(tmax, F(-np.inf))
    assert unclamped_bins([below], tmin, tmax, 3)[0] == 3                        # rounds up to bin tbins: clamped to the top bin
    big = (0.0, 8589934592.0)                                                    # a charge range that holds 2^32
    #            tmin   tmax  below  NaN     then one channel per charge edge, all at t = 1.0
    t = np.array([tmin, tmax, below, np.nan, 1, 1, 1, 1, 1, 1, 1, 1e9], np.float32)
    q = np.array([1.0, 1.0, 1.0, 1.0, -0.0, np.nan, -1.5, 4294967040.0, 4294967296.0, np.inf, 2.9, 1.0], np.float32)
    nch = len(t)
    got = dev_bin_hits(gpu, t, q, nch, 1, nch, 3, (tmin, tmax), 4, big)
    got = dev_bin_hits(gpu, t, q, nch, 1, nch, 3, (tmin, tmax), 4, big, *got)    # two calls accumulate
    want = bin_hits_loop(t, q, nch, 1, nch, 3, (tmin, tmax), 4, big)
    want = bin_hits_loop(t, q, nch, 1, nch, 3, (tmin, tmax), 4, big, *want)
    same_state(got, want)
    same_state(bin_hits_vec(t, q, nch, 1, nch, 3, (tmin, tmax), 4, big, *bin_hits_vec(t, q, nch, 1, nch, 3, (tmin, tmax), 4, big)), want)
    hc, hist = got
    assert hc.tolist() == [2, 0, 2, 0, 2, 2, 2, 2, 2, 2, 2, 0]                   # tmax, the NaN time and the sentinel are outside
    assert hist[0, 0, 0] == 2 and hist[2, 2, 0] == 2                             # tmin in bin 0, `below` in the clamped top bin
    for c in (4, 5, 6):                                                          # -0.0, NaN and -1.5 are charge 0
        assert hist[c, 0, 0] == 2
    assert hist[7, 0, 1] == 2                                                    # 4294967040 / 2^33 * 4 = 2 - 2^-23: bin 1
    assert hist[8, 0, 2] == 2 and hist[9, 0, 2] == 2                             # 2^32 and +inf saturate at 2^32 - 1 -> float 2^32
    assert hist[10, 0, 0] == 2 and hist.sum() == hc.sum()                        # 2.9 truncates to 2

    # a negative qmin with a zero charge; one bin each way
    got = dev_bin_hits(gpu, t, q, nch, 1, nch, 1, (tmin, tmax), 1, (-0.5, 9.5))
    same_state(got, bin_hits_loop(t, q, nch, 1, nch, 1, (tmin, tmax), 1, (-0.5, 9.5)))
    assert got[0].tolist() == [1, 0, 1, 0, 1, 1, 1, 0, 0, 0, 1, 0] and np.array_equal(got[1].reshape(-1), got[0])
    got = dev_bin_hits(gpu, t, q, nch, 1, nch, 3, (tmin, tmax), 2, (-3.0, 1.0))
    same_state(got, bin_hits_loop(t, q, nch, 1, nch, 3, (tmin, tmax), 2, (-3.0, 1.0)))
    assert got[1][4, 0, 1] == 1 and got[1][6, 0, 1] == 1                         # charge 0 in [-3, 1): (0 + 3) / 4 * 2 -> bin 1


def test_bin_hits_refusals_write_nothing(gpu):
    from chroma_amd import _lib
    t, q = np.full(4, 1.0, np.float32), np.full(4, 1.0, np.float32)
    marked_hc, marked_pdf = np.full(4, 7, np.uint32), np.full(4 * 2 * 2, 9, np.uint32)
    nan = float('nan')
    for tbins, trange, qbins, qrange in [(65536, (0.0, 2.0), 32768, (0.0, 2.0)),             # tbins * qbins = 2^31 > INT32_MAX
                                         (2, (nan, 2.0), 2, (0.0, 2.0)), (2, (0.0, nan), 2, (0.0, 2.0)),
                                         (2, (0.0, 2.0), 2, (nan, 2.0)), (2, (0.0, 2.0), 2, (0.0, nan))]:
        hc, hist = Guarded(gpu, marked_hc), Guarded(gpu, marked_pdf)
        dt, dq = gpu.to_gpu(t), gpu.to_gpu(q)
        with pytest.raises(_lib.ChromaError):
            _call(gpu, 'chroma_pdf_bin_hits', 4, 1, 4, dq.ptr, dt.ptr, tbins, trange[0], trange[1], qbins, qrange[0], qrange[1],
                  hc.ptr, hist.ptr)
        assert np.array_equal(hc.get(), marked_hc) and np.array_equal(hist.get(), marked_pdf)
    got = dev_bin_hits(gpu, t, q, 4, 1, 4, 2, (0.0, 2.0), 2, (0.0, 2.0), marked_hc, marked_pdf)          # the same arrays, accepted
    assert (got[0] == 8).all() and got[1].sum() == 9 * 16 + 4


# ---- eval_accumulate: the in-place rank merge --------------------------------------------------------------------
MERGE_K = [1, 2, 63, 64, 65, 100, 128, 129, 1000, 1023, 1024]
MERGE_NDAQ = [1, 63, 64, 65, 130]             # one round (partial, full) and more than one (64 + 1, 64 + 64 + 2)


@pytest.mark.parametrize('ndaq', MERGE_NDAQ)
@pytest.mark.parametrize('k', MERGE_K)
def test_eval_merge_random_tied_rows(gpu, k, ndaq):
    """Three carried calls over 41 channels (33 of them hit: 9 blocks of 4 waves, the last one partial): times on a 0.25
    grid, so old and new entries tie; the fraction of copies near the event time rises with the channel, so the running
    bin count crosses k early in some waves and never in others."""
    rng = np.random.default_rng(100000 + 1000 * ndaq + k)
    nch, stride = 41, 44
    hit, et, _ = mc_event(rng, nch, 1.0)
    hit[2::5] = False
    hit[-1] = True
    et[0] = 50.0
    near = np.linspace(0.0, 1.0, nch)
    got = want = ref = None
    use_ref = HAVE_REF and k + ndaq <= oracle.REF_PDF_TABLE_SIZE
    for call in range(3):
        t, _ = mc_channels(rng, nch, ndaq, stride, et, near)
        t[0::stride] = NOT_HIT                     # channel 0: one MC hit per call, outside its minimum bin
        t[0] = et[0] + F(7.25)
        got = dev_eval(gpu, hit, et, t, nch, ndaq, stride, 2.0, TRANGE, k, got)
        want = eval_accumulate_vec(hit, et, t, nch, ndaq, stride, 2.0, TRANGE, k, want)
        if use_ref:
            ref = oracle.ref_eval_accumulate(hit, et, t, nch, ndaq, stride, 2.0, TRANGE, k, ref)
    same_state(got, want)
    if use_ref:
        same_state(got, ref)
    assert (want[2][hit] < 1e8).any() and (want[2][~hit] == NOT_HIT).all() and not want[1][~hit].any()
    if 3 * ndaq >= 2 * k:
        assert (want[1][hit] >= k).any()
    assert want[1][0] == 0 and (want[2][0] < 1e8).sum() == min(k, 3)          # a part-filled table (k > 3)


def _designed_rows(k):
    """Channels of 130 copies (rounds of 64, 64 and 2) at event time 50, half width 1, with a chosen list and bin count
    before the call.  Returns (names, mc [130][n], bincount [n], nearest [n][k])."""
    ndaq = 130
    rows = []

    def row(name, old, new, bincount=0):
        """``old``: the list before (ascending, padded with 1e9 here); ``new``: {copy: distance from the event time}."""
        mc = np.full(ndaq, NOT_HIT, np.float32)
        for copy, d in new.items():
            mc[copy] = F(50.0) + F(d)
        tab = np.full(k, NOT_HIT, np.float32)
        old = np.sort(np.asarray(old, np.float32))[:k]
        tab[:len(old)] = old
        rows.append((name, mc, bincount, tab))

    ramp = lambda lo, hi, n: np.linspace(lo, hi, n).astype(np.float32)
    small = {j: 2.0 + 0.25 * j for j in range(64)}                 # 64 candidates in round 0, distances 2 .. 17.75
    row('all 64 new below a full list', ramp(30.0, 45.0, k), small)                 # everything moves up 64, the top 64 fall off
    row('all 64 new below a full list, round 1', ramp(30.0, 45.0, k), {64 + j: d for j, d in small.items()})
    row('all new above a full list', ramp(1.0, 1.75, k), small)                    # nothing changes
    row('new below a part-filled list', ramp(30.0, 45.0, max(1, k // 2)), small)
    ties = np.array([2.0 + 0.5 * (j % 4) for j in range(64)], np.float32)
    row('old equal to new throughout', np.tile(ties, k // 64 + 1)[:k], {j: ties[j] for j in range(64)})
    row('everything ties', np.full(k, 3.0, np.float32), {j: 3.0 for j in range(130)})
    row('everything ties, part-filled', np.full(max(1, k // 3), 3.0, np.float32), {j: 3.0 for j in range(130)})
    row('one candidate, round 0', ramp(5.0, 9.0, k), {37: 6.125})
    row('one candidate, round 1 only', ramp(5.0, 9.0, k), {64 + 5: 6.125})
    row('one candidate, last round, empty list', [], {129: 6.125})
    row('64 candidates in every full round', ramp(5.0, 9.0, max(1, k - 1)), {j: 4.0 + 0.03125 * ((j * 37) % 128) for j in range(128)})
    # the running bin count reaches k at a chosen copy: one in-bin hit there (distance 0.5), bincount k - 1 before;
    # every other copy is valid and outside the bin.  Copies before it are candidates, it and the later ones are not.
    for at in (0, 31, 63, 64, 127, 128):
        new = {j: 3.0 + 0.125 * ((j * 29) % 130) for j in range(130)}
        new[at] = 0.5
        row('bin count reaches k at copy %d' % at, ramp(10.0, 12.0, max(1, k // 2)), new, bincount=k - 1)
    # two in-bin hits short of k: the first in-bin copy is still a candidate, the second reaches k
    new = {j: 3.0 + 0.125 * ((j * 29) % 130) for j in range(130)}
    new[31], new[63], new[64] = 0.5, 0.25, 0.75
    row('in-bin copies 31 and 63, k - 2 before', [], new, bincount=max(0, k - 2))
    names = [r[0] for r in rows]
    return names, np.stack([r[1] for r in rows], axis=1), np.array([r[2] for r in rows], np.uint32), np.stack([r[3] for r in rows])


@pytest.mark.parametrize('k', MERGE_K)
def test_eval_merge_designed_rows(gpu, k):
    names, mc, bincount, nearest = _designed_rows(k)
    ndaq, nch = mc.shape
    hit, et = np.ones(nch, bool), np.full(nch, 50.0, np.float32)
    state = (np.arange(nch, dtype=np.uint32), bincount, nearest)
    t = np.ascontiguousarray(mc).reshape(-1)
    got = dev_eval(gpu, hit, et, t, nch, ndaq, nch, 2.0, TRANGE, k, state)
    want = eval_accumulate_vec(hit, et, t, nch, ndaq, nch, 2.0, TRANGE, k, state)
    same_state(eval_accumulate_loop(hit, et, t, nch, ndaq, nch, 2.0, TRANGE, k, state), want)
    for c, name in enumerate(names):                   # row by row, to name the one that differs
        assert got[0][c] == want[0][c] and got[1][c] == want[1][c], name
        assert np.array_equal(bits(got[2][c]), bits(want[2][c])), name
    if HAVE_REF and k + ndaq <= oracle.REF_PDF_TABLE_SIZE:
        same_state(got, oracle.ref_eval_accumulate(hit, et, t, nch, ndaq, nch, 2.0, TRANGE, k, state))
    # what the designed rows are for, by hand
    new = np.sort(np.array([2.0 + 0.25 * j for j in range(64)], np.float32))
    old = np.linspace(30.0, 45.0, k).astype(np.float32)
    moved = np.concatenate([new, old])[:k]
    assert np.array_equal(got[2][0], moved) and np.array_equal(got[2][1], moved)
    assert np.array_equal(bits(got[2][2]), bits(nearest[2])) and got[0][2] == 2 + 64
    assert (got[2][5] == 3.0).all() and got[0][5] == 5 + 130 and got[1][5] == 0
    assert (got[2][6] < 1e8).sum() == min(k, max(1, k // 3) + 130)
    for c, at in zip(range(11, 17), (0, 31, 63, 64, 127, 128)):
        assert got[1][c] == k and got[0][c] == c + 130, names[c]
        assert (got[2][c] < 1e8).sum() == min(k, max(1, k // 2) + at), names[c]             # the copies before `at`, no more
        assert not (got[2][c] == 0.5).any(), names[c]
    first_in_bin = (got[2][17] == 0.5).sum()
    assert got[1][17] == max(0, k - 2) + 3 and first_in_bin == (1 if k >= 2 else 0) and not (got[2][17] == 0.25).any()


@pytest.mark.parametrize('pattern', ['none', 'one', 'four', 'five of five', 'one of one'])
def test_eval_hit_counts_and_blocks(gpu, pattern):
    """nhit 0, 1, 4 and 5 (a block holds 4 waves); every channel hit, and a single one."""
    rng = np.random.default_rng(len(pattern))
    nch = {'five of five': 5, 'one of one': 1}.get(pattern, 9)
    hit = np.zeros(nch, bool)
    hit[{'none': [], 'one': [6], 'four': [0, 3, 4, 8], 'five of five': range(5), 'one of one': [0]}[pattern]] = True
    et = np.where(hit, 50.0, 1e9).astype(np.float32)
    ndaq, stride, k = 70, nch + 2, 65
    got = want = None
    for call in range(2):
        t, _ = mc_channels(rng, nch, ndaq, stride, et, np.full(nch, 0.3))
        got = dev_eval(gpu, hit, et, t, nch, ndaq, stride, 2.0, TRANGE, k, got)
        want = eval_accumulate_vec(hit, et, t, nch, ndaq, stride, 2.0, TRANGE, k, want)
    same_state(got, want)
    assert want[0].any() and want[1].any() == hit.any()


def test_eval_adversarial_hit_lists(gpu):
    """A listed id >= nchannels, and a listed id the event did not hit: that wave writes nothing."""
    rng = np.random.default_rng(77)
    nch, ndaq, k = 6, 70, 65
    hit = np.array([0, 0, 1, 1, 0, 1], bool)
    et = np.full(nch, 50.0, np.float32)
    t, _ = mc_channels(rng, nch, ndaq, nch, et, np.full(nch, 0.3))
    hit_list = [2, 7, 1, 3, 0xFFFFFFFF, 5]
    rows = np.full((len(hit_list) + 1, k), ROW_SENTINEL, np.float32)
    rows[[0, 3, 5]] = NOT_HIT
    hc, bc, rows = dev_eval_raw(gpu, hit, et, t, nch, ndaq, nch, 2.0, TRANGE, k, hit_list, np.zeros(nch, np.uint32),
                                np.zeros(nch, np.uint32), rows)
    want = eval_accumulate_vec(hit, et, t, nch, ndaq, nch, 2.0, TRANGE, k)
    assert np.array_equal(hc, want[0]) and np.array_equal(bc, want[1])                  # the unhit channel 1 is counted once
    assert np.array_equal(bits(rows[[0, 3, 5]]), bits(want[2][[2, 3, 5]])) and (rows[[0, 3, 5]] < 1e8).any()
    assert (rows[[1, 2, 4, 6]] == ROW_SENTINEL).all()


# ---- NaN is "not hit" ------------------------------------------------------------------------------------------------
def test_nan_mc_time_does_not_reach_the_sort(gpu):
    """k = 8, event time 50, MC times [10, NaN, 20, 30]: the NaN distance used to enter the bitonic network, whose
    fminf / fmaxf dropped it and duplicated its partner -- [20, 30, 40, 40, 1e9, ...] and a hit count of 4."""
    nch, k = 3, 8
    hit, et = np.array([1, 1, 0], bool), np.array([50.0, 50.0, 1e9], np.float32)
    mc = np.array([[10, 10, 10], [np.nan, 60, np.nan], [20, 20, 20], [30, 30, 30]], np.float32)
    got = dev_eval(gpu, hit, et, mc.reshape(-1), nch, 4, nch, 2.0, TRANGE, k)
    want = eval_accumulate_vec(hit, et, mc.reshape(-1), nch, 4, nch, 2.0, TRANGE, k)
    same_state(got, want)
    same_state(eval_accumulate_loop(hit, et, mc.reshape(-1), nch, 4, nch, 2.0, TRANGE, k), want)
    assert got[0].tolist() == [3, 4, 3] and got[1].tolist() == [0, 0, 0]
    assert got[2][0].tolist() == [20, 30, 40] + [1e9] * 5 and got[2][1].tolist() == [10, 20, 30, 40] + [1e9] * 4


@pytest.mark.parametrize('ndaq', [4, 130])
def test_nan_in_eval_accumulate(gpu, ndaq):
    """NaN MC times among valid ones, in and out of the minimum bin, over one round and three; a hit channel whose EVENT
    time is NaN keeps its bin count and a table of 1e9 while its valid MC hits are still counted."""
    rng = np.random.default_rng(ndaq)
    nch, stride, k = 13, 15, 9
    hit, et, _ = mc_event(rng, nch, 1.0)
    hit[3] = False
    et[[1, 7]] = np.nan
    got = want = None
    for call in range(2):
        t, _ = mc_channels(rng, nch, ndaq, stride, np.where(np.isnan(et), 50.0, et), np.full(nch, 0.3))
        t[rng.random(len(t)) < 0.2] = np.nan
        t[[0, 2]] = np.nan
        t[[1, 7]] = 60.0                           # the channels with a NaN event time have a valid MC hit
        got = dev_eval(gpu, hit, et, t, nch, ndaq, stride, 2.0, TRANGE, k, got)
        want = eval_accumulate_vec(hit, et, t, nch, ndaq, stride, 2.0, TRANGE, k, want)
    same_state(got, want)
    assert not np.isnan(got[2]).any()
    assert (got[2][[1, 7]] == NOT_HIT).all() and not got[1][[1, 7]].any() and got[0][[1, 7]].all()
    assert got[0].any() and got[1].any() and (got[2] < 1e8).any()


def test_nan_in_the_per_channel_kernels(gpu):
    nan = np.nan
    trange, qrange = (0.0, 100.0), (0.0, 10.0)
    #             ok   NaN t  NaN q  both   ok
    t = np.array([40, nan, 60, nan, 50, 40, 40, 40, 40, 40], np.float32)            # two copies of five channels
    q = np.array([2, 3, nan, nan, 4, 2, 3, 5, 6, nan], np.float32)
    nch, ndaq = 5, 2
    for time_only in (True, False):
        got = dev_moments(gpu, t, q, nch, ndaq, nch, trange, qrange, time_only)
        same_state(got, moments_vec(t, q, nch, ndaq, nch, trange, qrange, time_only))
        assert got[0].tolist() == ([2, 1, 2, 1, 2] if time_only else [2, 1, 1, 1, 1])
        assert all(np.isfinite(a).all() for a in got[1:])
        got = dev_moments(gpu, t, q, nch, ndaq, nch, trange, qrange, time_only, got)   # a NaN poisons nothing for the next call either
        assert all(np.isfinite(a).all() for a in got[1:]) and got[0][0] == 4
    # kernel_eval: NaN MC entries are not counted; a NaN EVENT time (channel 4) makes that channel's own sum NaN, no other
    hit = np.array([1, 1, 1, 0, 1], bool)
    et, eq = np.array([45, 45, 45, 1e9, nan], np.float32), np.array([2, 2, 2, 0, 2], np.float32)
    itb = np.full(nch, 0.5, np.float32)
    for time_only in (True, False):
        got = dev_kernel_eval(gpu, hit, et, eq, t, q, nch, ndaq, nch, trange, qrange, itb, itb, time_only)
        want = kernel_eval_vec(hit, et, eq, t, q, nch, ndaq, nch, trange, qrange, itb, itb, time_only)
        assert np.array_equal(got[0], want[0]) and got[0].tolist() == ([2, 1, 2, 1, 2] if time_only else [2, 1, 1, 1, 1])
        assert np.isnan(got[1][4]) and np.isnan(want[1][4])
        close_sums(got[1][:4], want[1][:4])
        close_sums(got[2][:4], want[2][:4])
        assert (got[1][:3] > 0).all() and got[1][3] == 0
    # the unhit channels of eval_accumulate (k_pdf_eval_hitcount) and bin_hits
    got = dev_eval(gpu, np.zeros(nch, bool), np.full(nch, 1e9, np.float32), t, nch, ndaq, nch, 2.0, trange, 3)
    assert got[0].tolist() == [2, 1, 2, 1, 2] and not got[1].any() and (got[2] == NOT_HIT).all()
    got = dev_bin_hits(gpu, t, q, nch, ndaq, nch, 4, trange, 2, (-0.5, 9.5))
    same_state(got, bin_hits_vec(t, q, nch, ndaq, nch, 4, trange, 2, (-0.5, 9.5)))
    assert got[0].tolist() == [2, 1, 2, 1, 2] and got[1][2, 2, 0] == 1 and got[1][4, 1, 0] == 1           # a NaN charge is charge 0


# ---- kernel_eval against float64 ------------------------------------------------------------------------------------
@pytest.mark.parametrize('i', range(len(KERNEL_CASES)))
def test_kernel_eval_accuracy(gpu, i):
    """KERNEL_CASES of tests/test_ref_pdf_host.py (t on both window ends, inverse bandwidths 0, 1e-4, 1, 1e3, charges on
    qmin and qmax), three carried calls: hit counts exact, sums within KERNEL_RTOL of float64 (see the module docstring)."""
    nch, ndaq, time_only = KERNEL_CASES[i]
    got = None
    for call, want in enumerate(kernel_reference(i)):
        case = kernel_case(nch, ndaq, time_only, call)
        got = dev_kernel_eval(gpu, *kernel_args(case), state=got)
        assert np.array_equal(got[0], want[0])
        close_sums(got[1], want[1])
        close_sums(got[2], want[2])
    assert time_only == (not got[2].any())
    assert (got[1] > KERNEL_ATOL).any() and not got[1][~case['hit']].any()
