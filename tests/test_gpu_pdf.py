"""The PDF kernels on the device against the NumPy restatements of tests/test_pdf_host.py (reference semantics:
chroma/cuda/pdf.cu), and the Simulation / Likelihood layer end to end on the demo detectors with photon bombs.
Counts and nearest-distance tables: exact; moments: bitwise; kernel values: 1e-5 relative to float64."""
import numpy as np
import pytest

from conftest import bomb
from test_pdf_host import (bin_hits_vec, eval_accumulate_vec, kernel_eval_vec, moments_vec, random_channels,
                           random_event)

pytestmark = pytest.mark.gpu

TRANGE, QRANGE = (0.0, 100.0), (-0.5, 9.5)


@pytest.fixture(scope='module')
def gpu():
    from chroma_amd import gpu as g
    ctx = g.create_cuda_context(0)
    yield g
    ctx.pop()


def channels(gpu, t, q, ndaq, stride):
    return gpu.GPUChannels(gpu.to_gpu(t), gpu.to_gpu(q), gpu.zeros(len(t), np.uint32), ndaq, stride)


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize('ndaq', [1, 63, 64, 65, 200])
def test_bin_hits(gpu, ndaq):
    rng = np.random.default_rng(100 + ndaq)
    nch, stride = 301, 320
    t, q = random_channels(rng, nch, ndaq, stride, trange=(-1.7, 7.3), quantum=0.01)
    t[:nch] = np.nextafter(np.float32(7.3), np.float32(-np.inf))            # rounds up to bin tbins unclamped
    q[:nch:2] = -1.5
    pdf = gpu.GPUPDF()
    pdf.setup_pdf(nch, 13, (-1.7, 7.3), 7, QRANGE)
    for _ in range(2):
        pdf.add_hits_to_pdf(channels(gpu, t, q, ndaq, stride))
    hc, hist = pdf.get_pdfs()
    want = bin_hits_vec(t, q, nch, ndaq, stride, 13, (-1.7, 7.3), 7, QRANGE)
    want = bin_hits_vec(t, q, nch, ndaq, stride, 13, (-1.7, 7.3), 7, QRANGE, *want)
    assert np.array_equal(hc, want[0]) and np.array_equal(hist, want[1])
    assert hist[:, 12, :].sum() >= nch and (hc == hist.sum(axis=(1, 2))).all()
    assert pdf.events_in_histogram == 2 * ndaq


@pytest.mark.parametrize('ndaq,k,frac_hit', [(1, 1, 0.5), (63, 320, 0.5), (64, 1024, 1.0), (65, 320, 0.0),
                                             (200, 320, 0.3), (200, 1, 1.0), (128, 1024, 0.5)])
def test_eval_accumulate(gpu, ndaq, k, frac_hit):
    rng = np.random.default_rng(ndaq * 7 + k)
    nch, stride = 257, 260
    hit, et, eq = random_event(rng, nch, frac_hit, trange=TRANGE)
    pdf = gpu.GPUPDF()
    pdf.setup_pdf_eval(hit, et, eq, 2.0, TRANGE, 1.0, QRANGE, min_bin_content=k)
    state = None
    for call in range(3):          # ties (times on a 0.25 grid), sentinels, t == tmin and tmax, carry-over between calls
        t, _ = random_channels(rng, nch, ndaq, stride, trange=TRANGE)
        pdf.accumulate_pdf_eval(channels(gpu, t, np.zeros_like(t), ndaq, stride))
        state = eval_accumulate_vec(hit, et, t, nch, ndaq, stride, 2.0, TRANGE, k, state)
    hc, value, uncert = pdf.get_pdf_eval()
    assert np.array_equal(hc, state[0])
    assert np.array_equal(pdf.eval_bincount_gpu.get(), state[1])
    assert np.array_equal(bits(pdf.get_nearest_mc()), bits(state[2]))
    if frac_hit == 0:
        assert not value.any() and hc.any()
    else:
        assert (value > 0).any()


def test_eval_accumulate_with_many_in_bin_and_few(gpu):
    """Channels that fill their minimum bin part-way through a round of 64 copies (the running count decides per lane)."""
    nch, ndaq, k = 64, 200, 37
    rng = np.random.default_rng(9)
    hit = np.ones(nch, bool)
    et = np.full(nch, 50.0, np.float32)
    t = np.where(rng.random(ndaq * nch) < 0.5, 50.0 + rng.integers(-3, 4, ndaq * nch) * 0.25,
                 rng.uniform(0, 100, ndaq * nch)).astype(np.float32)
    pdf = gpu.GPUPDF()
    pdf.setup_pdf_eval(hit, et, et, 1.0, TRANGE, 1.0, QRANGE, min_bin_content=k)
    pdf.accumulate_pdf_eval(channels(gpu, t, t, ndaq, nch))
    want = eval_accumulate_vec(hit, et, t, nch, ndaq, nch, 1.0, TRANGE, k)
    assert (want[1] >= k).any() and (want[1] < k).any()          # some channels fill their bin, some do not
    assert np.array_equal(pdf.eval_bincount_gpu.get(), want[1])
    assert np.array_equal(bits(pdf.get_nearest_mc()), bits(want[2]))


def test_carry_over_one_call_equals_many(gpu):
    """128 copies in one call == 2 x 64 == 128 x 1, bitwise, for every accumulator."""
    rng = np.random.default_rng(21)
    nch, ndaq = 300, 128
    hit, et, eq = random_event(rng, nch, 0.6, trange=TRANGE)
    t, q = random_channels(rng, nch, ndaq, nch, trange=TRANGE)
    itb = rng.uniform(0.05, 1.0, nch).astype(np.float32)
    results = []
    for per_call in (128, 64, 1):
        pdf = gpu.GPUPDF()
        pdf.setup_pdf_eval(hit, et, eq, 2.0, TRANGE, 1.0, QRANGE, min_bin_content=320)
        pdf.setup_pdf(nch, 10, TRANGE, 5, QRANGE)
        kern = gpu.GPUKernelPDF()
        kern.setup_moments(nch, TRANGE, (0.0, 10.0), time_only=False)
        mom = gpu.GPUKernelPDF()
        mom.setup_moments(nch, TRANGE, QRANGE, time_only=True)
        kern.setup_kernel(hit, et, eq)
        kern.inv_time_bandwidths_gpu = gpu.to_gpu(itb)
        kern.inv_charge_bandwidths_gpu = gpu.to_gpu(itb * 2)
        for first in range(0, ndaq, per_call):
            w = slice(first * nch, (first + per_call) * nch)
            ch = channels(gpu, t[w], q[w], per_call, nch)
            pdf.accumulate_pdf_eval(ch)
            pdf.add_hits_to_pdf(ch)
            mom.accumulate_moments(ch)
            kern.accumulate_kernel(ch)
        results.append([pdf.eval_hitcount_gpu.get(), pdf.eval_bincount_gpu.get(), bits(pdf.nearest_mc_gpu.get()),
                        pdf.get_pdfs()[1], mom.hitcount_gpu.get(), bits(mom.tmom1_gpu.get()), bits(mom.tmom2_gpu.get()),
                        kern.hitcount_gpu.get(), bits(kern.time_pdf_values_gpu.get()), bits(kern.charge_pdf_values_gpu.get())])
    for other in results[1:]:
        for a, b in zip(results[0], other):
            assert np.array_equal(a, b)


@pytest.mark.parametrize('time_only', [True, False])
@pytest.mark.parametrize('ndaq', [1, 65])
def test_moments_and_kernel_eval(gpu, time_only, ndaq):
    rng = np.random.default_rng(ndaq + 2 * time_only)
    nch, stride = 211, 224
    hit, et, eq = random_event(rng, nch, 0.5, trange=TRANGE)
    t, q = random_channels(rng, nch, ndaq, stride, trange=TRANGE)
    kern = gpu.GPUKernelPDF()
    kern.setup_moments(nch, TRANGE, (0.0, 10.0), time_only=time_only)
    ch = channels(gpu, t, q, ndaq, stride)
    kern.accumulate_moments(ch)
    kern.accumulate_moments(ch)
    want = moments_vec(t, q, nch, ndaq, stride, TRANGE, (0.0, 10.0), time_only)
    want = moments_vec(t, q, nch, ndaq, stride, TRANGE, (0.0, 10.0), time_only, want)
    got = [kern.hitcount_gpu.get(), kern.tmom1_gpu.get(), kern.tmom2_gpu.get(), kern.qmom1_gpu.get(), kern.qmom2_gpu.get()]
    assert np.array_equal(got[0], want[0])
    for a, b in zip(got[1:], want[1:]):
        assert np.array_equal(bits(a), bits(b))

    from chroma_amd.gpu.pdf import kernel_bandwidths
    kern.compute_bandwidth(hit, et, eq)
    want_itb, _ = kernel_bandwidths(*want[:3], et, time_only, *want[3:], eq)
    assert np.array_equal(bits(kern.inv_time_bandwidths_gpu.get()), bits(want_itb))
    assert (want_itb > 0).any() == (ndaq > 1)             # one copy, twice: no spread, no bandwidth
    # the kernel sums with bandwidths of every kind, zero (flat kernel) included
    itb = rng.uniform(0.02, 2.0, nch).astype(np.float32)
    itb[::5] = 0
    iqb = rng.uniform(0.1, 2.0, nch).astype(np.float32)
    kern.inv_time_bandwidths_gpu = gpu.to_gpu(itb)
    kern.inv_charge_bandwidths_gpu = gpu.to_gpu(iqb)
    kern.setup_kernel(hit, et, eq)
    kern.accumulate_kernel(ch)
    count, tv, qv = kernel_eval_vec(hit, et, eq, t, q, nch, ndaq, stride, TRANGE, (0.0, 10.0), itb, iqb, time_only)
    assert np.array_equal(kern.hitcount_gpu.get(), count)
    assert np.allclose(kern.time_pdf_values_gpu.get(), tv, rtol=1e-5, atol=1e-30)
    if not time_only:
        assert np.allclose(kern.charge_pdf_values_gpu.get(), qv, rtol=1e-5, atol=1e-30)
    assert (tv > 0).any()


def test_entry_points_refuse_bad_shapes(gpu):
    from chroma_amd import _lib
    ctx = gpu.get_context()
    lib = ctx._lib
    a = gpu.zeros(64, np.float32)
    u = gpu.zeros(64, np.uint32)
    with pytest.raises(_lib.ChromaError):
        _lib.check(lib.chroma_pdf_bin_hits(ctx.handle, 10, 1, 10, a.ptr, a.ptr, 0, 0.0, 1.0, 1, 0.0, 1.0, u.ptr, u.ptr))
    with pytest.raises(_lib.ChromaError):
        _lib.check(lib.chroma_pdf_bin_hits(ctx.handle, 10, 1, 10, a.ptr, a.ptr, 1, 1.0, 0.0, 1, 0.0, 1.0, u.ptr, u.ptr))
    with pytest.raises(_lib.ChromaError):
        _lib.check(lib.chroma_pdf_moments(ctx.handle, 1, 10, 2, 9, a.ptr, a.ptr, 0.0, 1.0, 0.0, 1.0, u.ptr, a.ptr, a.ptr, a.ptr, a.ptr))
    for k in (0, 1025):
        with pytest.raises(_lib.ChromaError):
            _lib.check(lib.chroma_pdf_eval_accumulate(ctx.handle, 10, 1, 10, u.ptr, a.ptr, a.ptr, 1, u.ptr, 1.0, 0.0, 1.0, k,
                                                      u.ptr, u.ptr, a.ptr))
    with pytest.raises(ValueError):
        gpu.GPUPDF().setup_pdf_eval(np.ones(4, bool), np.zeros(4), np.zeros(4), 1.0, TRANGE, 1.0, QRANGE, min_bin_content=1025)


# ---- end to end -----------------------------------------------------------------------------------------------
@pytest.fixture(scope='module', params=['tiny', 'detector_lite'])
def sim(request, gpu):
    from chroma_amd import demo
    from chroma_amd.loader import create_geometry_from_obj
    from chroma_amd.sim import Simulation
    det = create_geometry_from_obj(getattr(demo, request.param)())
    return Simulation(det, seed=11)


def _capture(obj, name, store):
    """Wrap obj.<name>(gpuchannels, ...) to keep a host copy of every channel array it is given."""
    original = getattr(obj, name)

    def wrapped(ch, *args, **kwargs):
        store.append((ch.t.get(), ch.q.get(), ch.ndaq, ch.stride))
        return original(ch, *args, **kwargs)
    setattr(obj, name, wrapped)


def test_simulation_pdfs_equal_the_restatement(sim):
    from chroma_amd import event
    assert sim._gpu_pdf is None and sim._gpu_pdf_kernel is None           # nothing made before first use
    nch = sim.detector.num_channels()
    bombs = [bomb(20000, seed=s) for s in (1, 2, 3)]

    seen = []
    _capture(sim.gpu_pdf, 'add_hits_to_pdf', seen)
    hitcount, pdf = sim.create_pdf(bombs, 100, (-0.5, 999.5), 10, (-0.5, 9.5), nreps=2)
    assert len(seen) == 6
    assert (hitcount > 0).any() and (pdf > 0).any()
    assert np.array_equal(hitcount, pdf.sum(axis=(1, 2)))
    want = None
    for t, q, ndaq, stride in seen:
        want = bin_hits_vec(t, q, nch, ndaq, stride, 100, (-0.5, 999.5), 10, (-0.5, 9.5), *(want or ()))
    assert np.array_equal(hitcount, want[0]) and np.array_equal(pdf, want[1])

    # the data event: one more bomb through the DAQ
    data = next(sim.simulate([bomb(20000, seed=99)], run_daq=True, keep_hits=False, keep_flat_hits=False))
    chans = data.channels
    assert chans.hit.any()

    seen = []
    _capture(sim.gpu_pdf, 'accumulate_pdf_eval', seen)
    hc, value, uncert = sim.eval_pdf(chans, bombs[:2], 1.0, (-0.5, 999.5), 1.0, (-0.5, 9.5), min_bin_content=20, nreps=2,
                                     ndaq=70, nscatter=2)
    assert sorted(s[2] for s in seen) == [6, 6, 6, 6, 64, 64, 64, 64]    # exactly ndaq acquisitions per copy, chunks <= 64
    state = None
    for t, q, ndaq, stride in seen:
        state = eval_accumulate_vec(chans.hit, chans.t, t, nch, ndaq, stride, 1.0, (-0.5, 999.5), 20, state)
    assert np.array_equal(hc, state[0])
    assert np.array_equal(bits(sim.gpu_pdf.get_nearest_mc()), bits(state[2]))
    from chroma_amd.gpu.pdf import pdf_eval_values
    want_value, _ = pdf_eval_values(chans.hit, state[0], state[1], state[2], 1.0, 20)
    assert np.array_equal(value, want_value) and (value[chans.hit] > 0).any()

    sim.setup_kernel(chans, bombs[:2], (-0.5, 999.5), (-0.5, 9.5), nreps=2, ndaq=3)
    itb = sim.gpu_pdf_kernel.inv_time_bandwidths_gpu.get()
    seen = []
    _capture(sim.gpu_pdf_kernel, 'accumulate_kernel', seen)
    hc, value, _ = sim.eval_kernel(chans, bombs[:2], (-0.5, 999.5), (-0.5, 9.5), nreps=2, ndaq=3)
    assert len(seen) == 4 and all(s[2] == 3 for s in seen)
    state = None
    for t, q, ndaq, stride in seen:
        state = kernel_eval_vec(chans.hit, chans.t, chans.q, t, q, nch, ndaq, stride, (-0.5, 999.5), (-0.5, 9.5), itb,
                                np.zeros_like(itb), True, state)
    assert np.array_equal(hc, state[0])
    assert np.allclose(value, state[1] / np.maximum(1, state[0]), rtol=1e-5, atol=1e-30)
    assert (value[chans.hit] > 0).any()

    with pytest.raises(NotImplementedError):
        sim.create_pdf([event.Event()], 10, (0, 1), 1, (0, 1))


def test_event_with_no_hit_channel(sim):
    nch = sim.detector.num_channels()
    from chroma_amd.event import Channels
    chans = Channels(np.zeros(nch, bool), np.full(nch, 1e9, np.float32), np.zeros(nch, np.float32))
    hc, value, uncert = sim.eval_pdf(chans, [bomb(5000, seed=4)], 1.0, (-0.5, 999.5), 1.0, (-0.5, 9.5), min_bin_content=5,
                                     ndaq=2)
    assert not value.any() and not uncert.any() and hc.any()


def test_likelihood_prefers_the_true_position(sim):
    from chroma_amd.likelihood import Likelihood
    if sim.detector.num_channels() > 1000:
        pytest.skip('one detector is enough')
    data = next(sim.simulate([bomb(20000, seed=123)], run_daq=True, keep_hits=False, keep_flat_hits=False))
    like = Likelihood(sim, data, trange=(-0.5, 999.5))

    def bombs(pos, seed):
        for i in range(100):
            yield bomb(20000, seed=seed + i, pos=pos)
    nll_true = like.eval(bombs((0, 0, 0), 1000), 3, nreps=4, ndaq=16)
    nll_off = like.eval(bombs((1000.0, 0, 0), 2000), 3, nreps=4, ndaq=16)
    assert np.isfinite(nll_true.nominal_value) and np.isfinite(nll_off.nominal_value)
    assert nll_true.nominal_value < nll_off.nominal_value, (nll_true, nll_off)
