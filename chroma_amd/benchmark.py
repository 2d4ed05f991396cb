"""The reference's own timing harness for this path (chroma/benchmark.py:22-96): ``intersect``
(ray intersections per second through distance_to_mesh), ``load_photons`` (host -> device photon
upload rate), ``propagate`` (photons per second, default max_steps=10, Morton-sorted isotropic
bomb of U(400, 800) nm photons), ``pdf`` (events histogrammed per second), ``pdf_eval`` (events
accumulated into a PDF evaluation per second) and ``hybrid_render`` (the camera's hybrid mode: triangle samples
and image rays per second).  Returns (mean, std) of the rate instead of an
``uncertainties.ufloat`` (that package is not a dependency here).  ``pdf`` and ``pdf_eval`` take a photon
bomb of ``nphotons`` at the centre as their event, in place of the reference's GEANT4 100 MeV electron.
"""
import ctypes
import time

import numpy as np

from chroma_amd import _lib, event, gpu, sample, tools
from chroma_amd.transform import normalize


def _rate(nphotons, run_times):
    t = np.asarray(run_times)
    mean = nphotons / t.mean()
    return mean, mean * (t.std() / t.mean())


def intersect(gpu_geometry, number=100, nphotons=500000, nthreads_per_block=64, max_blocks=1024):
    "Average number of ray intersections per second (mean, std)."
    ctx = gpu_geometry.ctx
    distances = gpu.empty(nphotons, np.float32, ctx)
    run_times = []
    for i in range(number):
        pos = gpu.zeros(3 * nphotons, np.float32, ctx)
        d = sample.uniform_sphere(nphotons)
        d = gpu.to_gpu(np.ascontiguousarray(d[tools.argsort_direction(d)], dtype=np.float32).reshape(-1), ctx)
        ctx.synchronize()
        t0 = time.time()
        _lib.check(ctx._lib.chroma_distance_to_mesh(ctx.handle, gpu_geometry.handle, nphotons, pos.ptr, d.ptr, distances.ptr, None))
        ctx.synchronize()
        if i > 0:       # the first call pays one-off costs
            run_times.append(time.time() - t0)
    return _rate(nphotons, run_times)


def _bomb(nphotons):
    pos = np.zeros((nphotons, 3))
    d = sample.uniform_sphere(nphotons)
    d = d[tools.argsort_direction(d)]
    pol = normalize(np.cross(sample.uniform_sphere(nphotons), d))
    return event.Photons(pos, d, pol, np.random.uniform(400, 800, size=nphotons))


def load_photons(number=100, nphotons=500000):
    "Average number of photons moved to device memory per second (mean, std)."
    photons = _bomb(nphotons)
    ctx = gpu.get_context()
    run_times = []
    for i in range(number):
        t0 = time.time()
        gp = gpu.GPUPhotons(photons)
        ctx.synchronize()
        if i > 0:
            run_times.append(time.time() - t0)
        del gp
    return _rate(nphotons, run_times)


def propagate(gpu_detector, number=10, nphotons=500000, nthreads_per_block=64, max_blocks=1024):
    "Average number of photons propagated per second (mean, std); photons resident when the clock starts."
    rng_states = gpu.get_rng_states(nthreads_per_block * max_blocks)
    ctx = gpu_detector.ctx
    run_times = []
    for i in range(number):
        gp = gpu.GPUPhotons(_bomb(nphotons))
        ctx.synchronize()
        t0 = time.time()
        gp.propagate(gpu_detector, rng_states, nthreads_per_block, max_blocks)
        ctx.synchronize()
        if i > 0:
            run_times.append(time.time() - t0)
        del gp
    return _rate(nphotons, run_times)


def pdf(gpu_detector, npdfs=10, nevents=100, nreps=16, ndaq=1, nphotons=20000, nthreads_per_block=64, max_blocks=1024):
    """Events histogrammed per second (mean, std) (chroma/benchmark.py:98-150): ``nevents`` bombs, each propagated
    ``nreps`` times, each copy through ``ndaq`` DAQ acquisitions (one GPUDaq(ndaq) call) binned into (100 x 10)-bin
    time and charge histograms per channel."""
    ctx = gpu_detector.ctx
    rng_states = gpu.get_rng_states(nthreads_per_block * max_blocks)
    gpu_daq = gpu.GPUDaq(gpu_detector, ndaq=ndaq)
    gpu_pdf = gpu.GPUPDF(ctx)
    gpu_pdf.setup_pdf(gpu_detector.nchannels, 100, (-0.5, 999.5), 10, (-0.5, 9.5))
    photons = _bomb(nphotons)
    run_times = []
    for i in range(npdfs):
        t0 = time.time()
        gpu_pdf.clear_pdf()
        for _ in range(nevents):
            gpu_photons = gpu.GPUPhotons(photons, ncopies=nreps)
            gpu_photons.propagate(gpu_detector, rng_states, nthreads_per_block, max_blocks)
            for gpu_photon_slice in gpu_photons.iterate_copies():
                gpu_daq.begin_acquire()
                gpu_daq.acquire(gpu_photon_slice, rng_states, nthreads_per_block, max_blocks)
                gpu_pdf.add_hits_to_pdf(gpu_daq.end_acquire(), nthreads_per_block)
        gpu_pdf.get_pdfs()
        if i > 0:       # the first pass pays one-off costs
            run_times.append(time.time() - t0)
    return _rate(nevents * nreps * ndaq, run_times)


def pdf_eval(gpu_detector, npdfs=10, nevents=25, nreps=16, ndaq=128, nphotons=20000, nthreads_per_block=64,
             max_blocks=1024):
    """Events accumulated into a PDF evaluation per second (mean, std) (chroma/benchmark.py:152-232): one bomb
    through the DAQ is the data event; ``nevents`` bombs, each propagated ``nreps`` times, each copy's detected
    photons through ``ndaq`` DAQ acquisitions (GPUDaq chunks of at most 64 copies, one accumulate call each)."""
    ctx = gpu_detector.ctx
    rng_states = gpu.get_rng_states(nthreads_per_block * max_blocks)
    photons = _bomb(nphotons)
    data_photons = gpu.GPUPhotons(photons)
    data_photons.propagate(gpu_detector, rng_states, nthreads_per_block, max_blocks)
    data_daq = gpu.GPUDaq(gpu_detector)
    data_daq.begin_acquire()
    data_daq.acquire(data_photons, rng_states, nthreads_per_block, max_blocks)
    data_channels = data_daq.end_acquire().get()

    daqs = [gpu.GPUDaq(gpu_detector, ndaq=min(64, ndaq - first)) for first in range(0, ndaq, 64)]
    gpu_pdf = gpu.GPUPDF(ctx)
    gpu_pdf.setup_pdf_eval(data_channels.hit, data_channels.t, data_channels.q, 0.05, (-0.5, 999.5), 1.0, (-0.5, 20),
                           min_bin_content=20, time_only=True)
    run_times = []
    for i in range(npdfs):
        t0 = time.time()
        gpu_pdf.clear_pdf_eval()
        for _ in range(nevents):
            gpu_photons = gpu.GPUPhotons(photons, ncopies=nreps)
            gpu_photons.propagate(gpu_detector, rng_states, nthreads_per_block, max_blocks)
            for gpu_photon_slice in gpu_photons.iterate_copies():
                detected = gpu_photon_slice.select(event.SURFACE_DETECT)
                for gpu_daq in daqs:
                    gpu_daq.begin_acquire()
                    gpu_daq.acquire(detected, rng_states, nthreads_per_block, max_blocks)
                    gpu_pdf.accumulate_pdf_eval(gpu_daq.end_acquire(), nthreads_per_block)
        gpu_pdf.get_pdf_eval()
        if i > 0:
            run_times.append(time.time() - t0)
    return _rate(nevents * nreps * ndaq, run_times)


def hybrid_render(gpu_geometry, number=5, size=(800, 600), source_position=None, max_steps=10, seed=1):
    """The camera's hybrid mode (GPUHybridRender; chroma/camera.py:188-249) from the camera's initial view: ((triangle
    samples per second of one update_xyz_lookup: 3 wavelengths x every triangle), (image rays per second of one
    update_image: 3 wavelengths x every pixel)), each (mean, std) over ``number`` timed passes after one untimed one.
    The source sits at the camera unless ``source_position`` is given.  ``gpu_geometry`` must keep its Geometry."""
    from chroma_amd.render_cli import camera_rays
    ctx = gpu_geometry.ctx
    point, pos, dirs = camera_rays(gpu_geometry.geometry, size)
    rays = gpu.GPURays(pos, dirs, max_alpha_depth=1)
    renderer = gpu.GPUHybridRender(gpu_geometry, rays, seed=seed, max_steps=max_steps)
    source = point if source_position is None else source_position
    lookup_times, image_times = [], []
    for i in range(number + 1):
        ctx.synchronize()
        t0 = time.time()
        renderer.clear_xyz_lookup()
        renderer.update_xyz_lookup(source)
        ctx.synchronize()
        t1 = time.time()
        renderer.clear_image()
        renderer.update_image()
        renderer.process_image()
        ctx.synchronize()
        t2 = time.time()
        if i > 0:
            lookup_times.append(t1 - t0)
            image_times.append(t2 - t1)
    return (_rate(3 * renderer.ntriangles, lookup_times), _rate(3 * renderer.npixels, image_times))
