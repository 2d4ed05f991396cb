"""What PMT dark noise adds to the time-binned DAQ of one chunk of a large detector:

    python tools/daq_noise_probe.py [--repeats 5] [--label NAME] [--events 578] [--channels 29007] [--photons 1000000] [--rates 1e3,1e4]

The DAQ reads of a detector only which channel a triangle belongs to, so the detector here is a stand-in that is quick to build:
``--channels`` small boxes on a grid, each a PMT with the demo's time and charge distributions.  The photons are made here from a
seed and never propagated: ``--photons`` over ``--events`` events of equal size, each on a uniformly drawn triangle, three in ten
detected, at times uniform over the window -- 1000 bins of 1 ns from 0 on, one chunk of ``GPUEventDaq``.

Per dark rate (0 Hz, the call without noise, first; then ``--rates`` per channel), ``--repeats`` times after one warm-up:
``GPUEventDaq.acquire_pulses`` by the host clock (it ends with its results on the host), and inside it the clock around the two
library calls.  Then the noise kernels as alone as the library runs them: the counting call on an EMPTY photon span
(k_daq_noise_count, a 16-byte clear and read-back) and the acquiring call on it (both noise kernels, then the sort and the
reductions of the noise alone).  The comparison is with the call without noise in the same run, never with an expectation; a kernel
trace of this script gives the kernels' own times."""
import argparse
import ctypes
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

import numpy as np

from chroma_amd import event, gpu, make
from chroma_amd.demo.optics import water, black_surface
from chroma_amd.detector import Detector
from chroma_amd.geometry import Solid
from chroma_amd.loader import create_geometry_from_obj

from daq_pulses_probe import Clocked


def stand_in(nchannels):
    """``nchannels`` boxes of 10 mm on a grid of 100 mm, every one a channel."""
    geo = Detector(water)
    pmt = Solid(make.cube(10.0), water, water, surface=black_surface)
    side = int(np.ceil(nchannels ** (1.0 / 3.0)))
    for k in range(nchannels):
        geo.add_pmt(pmt, displacement=100.0 * np.array([k % side, k // side % side, k // (side * side)], dtype=np.float64))
    geo.set_time_dist_gaussian(1.5, -7.5, 7.5)
    geo.set_charge_dist_gaussian(1.0, 0.1, 0.0, 1.5)
    return create_geometry_from_obj(geo)


def made_photons(n, ntriangles, window, seed=7):
    rng = np.random.default_rng(seed)
    pos = np.zeros((n, 3), dtype=np.float32)
    direction = np.tile(np.array([0.0, 0.0, 1.0], dtype=np.float32), (n, 1))
    pol = np.tile(np.array([1.0, 0.0, 0.0], dtype=np.float32), (n, 1))
    flags = np.where(rng.random(n) < 0.3, event.SURFACE_DETECT, event.SURFACE_ABSORB).astype(np.uint32)
    return event.Photons(pos, direction, pol, np.full(n, 400.0, dtype=np.float32),
                         t=rng.uniform(window[0], window[0] + window[1] * window[2], n).astype(np.float32),
                         last_hit_triangles=rng.integers(0, ntriangles, n).astype(np.int32), flags=flags)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--label', default='')
    ap.add_argument('--events', type=int, default=578)
    ap.add_argument('--channels', type=int, default=29007)
    ap.add_argument('--photons', type=int, default=1000000)
    ap.add_argument('--rates', default='1e3,1e4', help='dark rates per channel, Hz')
    args = ap.parse_args()
    window = (0.0, 1.0, 1000)
    t0 = time.perf_counter()
    detector = stand_in(args.channels)
    ctx = gpu.create_cuda_context(0)
    gpu_detector = gpu.GPUDetector(detector)
    daq = gpu.GPUEventDaq(gpu_detector, max_entries=args.events * args.channels)
    assert daq.rows_per_chunk == args.events
    photons = gpu.GPUPhotons(made_photons(args.photons, len(detector.mesh.triangles), window))
    rng_states = gpu.get_rng_states(1, seed=5)
    bounds = (np.arange(args.events + 1, dtype=np.int64) * args.photons) // args.events
    nothing = np.zeros(args.events + 1, dtype=np.int64)
    lib = ctx._lib
    calls = {}
    for name in ('chroma_daq_count_pulses', 'chroma_daq_acquire_pulses', 'chroma_daq_count_pulses_noise', 'chroma_daq_acquire_pulses_noise'):
        calls[name] = Clocked(getattr(lib, name))
        setattr(lib, name, calls[name])
    print('# %s  GPUEventDaq.acquire_pulses, one chunk of %d events x %d channels (%.3g words), %d photons, window %r, %d repeats after one '
          'warm-up (stand-in detector and photons made in %.0f s); ms, median (min .. max)'
          % (args.label, args.events, args.channels, args.events * args.channels, args.photons, window, args.repeats, time.perf_counter() - t0))
    print('# dark rate, Hz | mu per word |        acquire_pulses         | count call | acquire call | rest | the same on an empty photon span: '
          'count call | acquire call | pulses | photoelectrons | of them noise')
    cell = lambda ts: '%8.2f (%7.2f .. %7.2f)' % (statistics.median(ts), min(ts), max(ts))
    for rate in [0.0] + [float(x) for x in args.rates.split(',')]:
        noise = gpu.DaqNoise(rate)
        suffix = '' if noise.off else '_noise'
        count, acquire = calls['chroma_daq_count_pulses' + suffix], calls['chroma_daq_acquire_pulses' + suffix]
        times = {'pulses': [], 'count': [], 'call': [], 'empty count': [], 'empty call': []}
        for repeat in range(args.repeats + 1):
            count.ms = acquire.ms = 0.0
            t1 = time.perf_counter()
            pulses = daq.acquire_pulses(photons, rng_states, bounds, window, acquisition=0, noise=noise)
            t2 = time.perf_counter()
            took = (1e3 * (t2 - t1), count.ms, acquire.ms)
            count.ms = acquire.ms = 0.0
            daq.acquire_pulses(photons, rng_states, nothing, window, acquisition=0, noise=noise)
            if repeat:
                for key, ms in zip(('pulses', 'count', 'call', 'empty count', 'empty call'), took + (count.ms, acquire.ms)):
                    times[key].append(ms)
        med = {k: statistics.median(v) for k, v in times.items()}
        print('%14.0f | %11.3g | %s | %10.2f | %12.2f | %4.2f | %10.2f | %12.2f | %d | %d | %d'
              % (rate, noise.mu(window), cell(times['pulses']), med['count'], med['call'], med['pulses'] - med['count'] - med['call'],
                 med['empty count'], med['empty call'], len(pulses.channel), int(pulses.npe.sum(dtype=np.uint64)), int(pulses.noise.sum(dtype=np.uint64))), flush=True)
    ctx.pop()


if __name__ == '__main__':
    main()
