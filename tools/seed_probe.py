"""What seeding a batch of firings costs on the device and on the host:

    python tools/seed_probe.py [--repeats 5] [--window 1.0] [--sizes 8x100,256x500,2048x2000] [--host-fits 4] [--channels 2000] [--radius 8000]
                               [--speed 200] [--sigma 1.0] [--levels 6]

A synthetic batch per size FITSxHITS: ``--channels`` channels on a sphere of ``--radius`` mm, per fit a vertex inside half the
radius and a time, HITS hits on random channels at the straight-line time of flight plus a Gaussian of ``--sigma`` ns, a tenth
of them uniformly random in time (noise).  The default ``VertexSeeder`` (a grid of radius / 8: 2109 candidates; six levels).
chroma_vertex_seed is timed on the whole batch, hit arrays resident, after one warm-up, by the host clock around the call (it
returns with its outputs written), as many times as fill ``--window`` seconds and ``--repeats`` times at the least;
chroma_vertex_seed_host -- ONE thread, plain loops -- on the first ``--host-fits`` fits of the same batch (the fits of a batch cost
the same: same hits, same candidates, same levels), over a window of its own, and its fits
are compared with the device's bit for bit.  Prints per size the medians (min .. max), fits per second and hit evaluations per
second of both -- an evaluation is one hit at one position: hits x (candidates + 125 levels + 1) per fit -- and how far the seeds
lie from the vertices the hits were made at.  Seeds of simulated light are not looked at here."""
import argparse
import ctypes
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

import numpy as np

from chroma_amd import _lib, gpu
from chroma_amd.gpu.seed import GPUVertexSeeder
from chroma_amd.gpu.tools import to_gpu, zeros
from chroma_amd.seed import VertexSeeder


def sphere(n, radius):
    k = np.arange(n) + 0.5
    polar, azimuth = np.arccos(1.0 - 2.0 * k / n), np.pi * (1.0 + 5.0 ** 0.5) * k
    return radius * np.stack([np.sin(polar) * np.cos(azimuth), np.sin(polar) * np.sin(azimuth), np.cos(polar)], axis=1)


def make_batch(rng, positions, nfits, nhits, radius, speed, sigma):
    direction = rng.normal(size=(nfits, 3))
    truth = direction / np.linalg.norm(direction, axis=1)[:, None] * (0.5 * radius * rng.uniform(size=(nfits, 1)) ** (1.0 / 3.0))
    t_true = rng.uniform(-100.0, 100.0, size=nfits)
    channel = rng.integers(0, len(positions), size=(nfits, nhits))
    t = t_true[:, None] + np.linalg.norm(positions[channel] - truth[:, None, :], axis=2) / speed + rng.normal(0.0, sigma, size=(nfits, nhits))
    noise = rng.uniform(size=(nfits, nhits)) < 0.1
    t[noise] = (t_true[:, None] + rng.uniform(-20.0, 2.0 * radius / speed + 20.0, size=(nfits, nhits)))[noise]
    return truth, t_true, np.arange(nfits + 1) * nhits, channel.reshape(-1), t.reshape(-1)


def summary(times):
    return '%9.3f ms (%.3f .. %.3f, %d calls)' % (1e3 * statistics.median(times), 1e3 * min(times), 1e3 * max(times), len(times))


def clocked(call, before, repeats, window):
    """the times of ``call``, each after ``before()``: ``repeats`` of them at the least, and as many as fill ``window`` seconds"""
    times = []
    while len(times) < repeats or (sum(times) < window and len(times) < 20000):
        before()
        start = time.perf_counter()
        call()
        times.append(time.perf_counter() - start)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--window', type=float, default=1.0, help='seconds of timed calls per size and side, at the least')
    ap.add_argument('--sizes', default='8x100,256x500,2048x2000')
    ap.add_argument('--host-fits', type=int, default=4)
    ap.add_argument('--channels', type=int, default=2000)
    ap.add_argument('--radius', type=float, default=8000.0)
    ap.add_argument('--speed', type=float, default=200.0)
    ap.add_argument('--sigma', type=float, default=1.0)
    ap.add_argument('--levels', type=int, default=6)
    args = ap.parse_args()
    ctx = gpu.create_cuda_context(0)
    positions = sphere(args.channels, args.radius)
    seeder = VertexSeeder(positions, args.speed, levels=args.levels)
    runner = GPUVertexSeeder(ctx, seeder)
    ncand = len(seeder.cand)
    per_hit = ncand + 125 * seeder.levels + 1
    print('seed probe: %d channels, %d candidates, %d levels, %d positions per fit; host twin on ONE thread' % (args.channels, ncand, seeder.levels, per_hit))
    rng = np.random.default_rng(5)
    p = lambda a: None if a is None else ctypes.c_void_p(a.ptr)
    for size in args.sizes.split(','):
        nfits, nhits = [int(x) for x in size.split('x')]
        truth, t_true, offsets, channel, t = make_batch(rng, positions, nfits, nhits, args.radius, args.speed, args.sigma)
        prepared = seeder.prepare(offsets, channel, t)
        out = seeder.outputs(nfits, False)
        hits = [to_gpu(a, ctx=ctx) for a in (prepared.channel, prepared.time, prepared.weight)]
        d_out = [None if a is None else zeros(a.size, a.dtype, ctx=ctx) for a in out]

        def device():
            _lib.check(ctx._lib.chroma_vertex_seed(ctx.handle, ctypes.byref(prepared.struct), seeder.nchannels, p(runner.channel_pos), ncand, p(runner.cand),
                                                   nfits, _lib.ptr(prepared.offsets), _lib.ptr(prepared.tau0), *([p(a) for a in hits] + [p(a) for a in d_out])),
                       ctx._lib)

        device()
        times = clocked(device, ctx.synchronize, args.repeats, args.window)
        got = [None if a is None else d.get().reshape(a.shape) for a, d in zip(out, d_out)]
        fits = seeder.finish(prepared, got)
        # the host twin on the first fits
        nhost = min(nfits, args.host_fits)
        part = seeder.prepare(offsets[:nhost + 1], channel[:nhost * nhits], t[:nhost * nhits])
        part.struct = prepared.struct          # (the batch's bins)
        want = seeder.run_host(part)
        host_times = clocked(lambda: seeder.run_host(part), lambda: None, max(1, args.repeats // 2), args.window)
        same = all(a is None or np.array_equal(a, b[:nhost]) for a, b in zip(want, got))
        evals = float(nhits) * per_hit
        dev, hst = statistics.median(times), statistics.median(host_times) / nhost
        miss = np.linalg.norm(fits.pos - truth, axis=1)
        print('%5d fits x %5d hits, %d bins: device %s = %10.0f fits/s %.3e evaluations/s | host %s for %d fits = %8.1f fits/s %.3e evaluations/s | x %.1f | '
              'first %d fits the same: %s' % (nfits, nhits, prepared.struct.nbins, summary(times), nfits / dev, nfits * evals / dev, summary(host_times), nhost,
                                              1.0 / hst, evals / hst, hst * nfits / dev, nhost, same))
        print('      seed - truth: median %.1f mm, 90%% %.1f mm, worst %.1f mm; t0 - truth: median %.2f ns; hits outside: %.1f %%'
              % (np.median(miss), np.percentile(miss, 90), miss.max(), np.median(fits.t0 - t_true), 100.0 * fits.outside.sum() / max(1, fits.nhits.sum())))
        if not same:
            return 1
    return 0


if __name__ == '__main__':
    sys.exit(main())
