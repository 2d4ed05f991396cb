"""What seeding the directions of a batch of firings costs on the device and on the host, and how far the seeded axes lie from
the truth on synthetic rings:

    python tools/dirseed_probe.py [--repeats 5] [--window 1.0] [--sizes 1x100x864,8x100x864,256x500x864,2048x2000x864,256x500x3456]
                                  [--host-fits 4] [--channels 2000] [--radius 8000] [--cos 0.75] [--sigma 0.03] [--levels 6]

A synthetic batch per size FITSxHITSxCANDIDATES (CANDIDATES = 6 grid^2: 864 is grid 12, 3456 grid 24): ``--channels`` channels on
a sphere of ``--radius`` mm, per fit a vertex inside half the radius and an axis; HITS unit-weight hits on the channels whose
cosine to the axis, seen from the vertex, is nearest to a draw from a Gaussian of ``--sigma`` about ``--cos``, a tenth of them on
random channels instead (noise).  The vertex is given exactly (no vertex seed runs) and no time cut is made: the hit arrays hold
channel and weight.  ``DirectionSeeder(cherenkov_profile(cos, max(sigma, 0.03)), grid, levels)``.  chroma_direction_seed is timed
on the whole batch, hit arrays, vertices and bins resident, after one warm-up, by the host clock around the call (it returns with
its outputs written), as many times as fill ``--window`` seconds and ``--repeats`` times at the least; chroma_direction_seed_host
-- ONE thread, plain loops -- on the first ``--host-fits`` fits of the same batch, over a window of its own, and its fits are
compared with the device's bit for bit.  Prints per size the medians (min .. max), fits per second and hit evaluations per second
of both -- an evaluation is one hit at one direction: hits x (candidates + 125 levels) per fit -- and the angle between the
seeded axes and the true ones.  Seeds of simulated light are not looked at here."""
import argparse
import ctypes
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

import numpy as np

from chroma_amd import _lib, gpu
from chroma_amd.gpu.seed import GPUDirectionSeeder
from chroma_amd.gpu.tools import to_gpu, zeros
from chroma_amd.seed import DirectionSeeder, SeedFits, VertexSeeder


def sphere(n, radius):
    k = np.arange(n) + 0.5
    polar, azimuth = np.arccos(1.0 - 2.0 * k / n), np.pi * (1.0 + 5.0 ** 0.5) * k
    return radius * np.stack([np.sin(polar) * np.cos(azimuth), np.sin(polar) * np.sin(azimuth), np.cos(polar)], axis=1)


def unit(v):
    return v / np.linalg.norm(v, axis=-1)[..., None]


def make_batch(rng, positions, nfits, nhits, radius, cos_c, sigma):
    vertex = unit(rng.normal(size=(nfits, 3))) * (0.5 * radius * rng.uniform(size=(nfits, 1)) ** (1.0 / 3.0))
    axis = unit(rng.normal(size=(nfits, 3)))
    channel = np.empty((nfits, nhits), dtype=np.int64)
    for f in range(nfits):
        cosine = unit(positions - vertex[f]) @ axis[f]
        order = np.argsort(cosine)
        wanted = np.clip(rng.normal(cos_c, sigma, size=nhits), -1.0, 1.0)
        channel[f] = order[np.clip(np.searchsorted(cosine[order], wanted), 0, len(order) - 1)]
    noise = rng.uniform(size=(nfits, nhits)) < 0.1
    channel[noise] = rng.integers(0, len(positions), size=(nfits, nhits))[noise]
    return vertex, axis, np.arange(nfits + 1) * nhits, channel.reshape(-1)


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


def seeds_at(vertex_seeder, vertex):
    """the ``SeedFits`` whose positions are ``vertex`` (mm), rounded to position units"""
    n = len(vertex)
    pos_int = np.floor(vertex / vertex_seeder.unit + 0.5).astype(np.int32)
    zero = np.zeros(n, dtype=np.uint32)
    return SeedFits(pos_int * vertex_seeder.unit, np.zeros(n), zero, zero, zero, np.zeros((n, 1), dtype=np.uint32), zero, zero, pos_int)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--window', type=float, default=1.0, help='seconds of timed calls per size and side, at the least')
    ap.add_argument('--sizes', default='1x100x864,8x100x864,256x500x864,2048x2000x864,256x500x3456')
    ap.add_argument('--host-fits', type=int, default=4)
    ap.add_argument('--channels', type=int, default=2000)
    ap.add_argument('--radius', type=float, default=8000.0)
    ap.add_argument('--cos', type=float, default=0.75)
    ap.add_argument('--sigma', type=float, default=0.03)
    ap.add_argument('--levels', type=int, default=6)
    args = ap.parse_args()
    ctx = gpu.create_cuda_context(0)
    positions = sphere(args.channels, args.radius)
    vertex_seeder = VertexSeeder(positions, 200.0, pos_unit_mm=0.5)
    print('direction seed probe: %d channels, ring at cos %.3f +- %.3f, %d levels; host twin on ONE thread' % (args.channels, args.cos, args.sigma, args.levels))
    rng = np.random.default_rng(5)
    p = lambda a: None if a is None else ctypes.c_void_p(a.ptr)
    runners = {}
    for size in args.sizes.split(','):
        nfits, nhits, ncand = [int(x) for x in size.split('x')]
        grid = int(round(math.sqrt(ncand / 6.0)))
        if 6 * grid * grid != ncand:
            ap.error('CANDIDATES is 6 grid^2 (%d is not)' % ncand)
        if grid not in runners:
            seeder = DirectionSeeder(vertex_seeder, profile=DirectionSeeder.cherenkov_profile(args.cos, max(args.sigma, 0.03)), grid=grid, levels=args.levels)
            runners[grid] = GPUDirectionSeeder(ctx, seeder)
        runner = runners[grid]
        seeder = runner.seeder
        per_hit = ncand + 125 * seeder.levels
        vertex, axis, offsets, channel = make_batch(rng, positions, nfits, nhits, args.radius, args.cos, args.sigma)
        seeds = seeds_at(vertex_seeder, vertex)
        prepared = seeder.prepare(seeds, offsets, channel)
        out = seeder.outputs(nfits, False)
        hits = [to_gpu(prepared.channel, ctx=ctx), None, to_gpu(prepared.weight, ctx=ctx)]
        d_vertex, d_bin = to_gpu(prepared.vertex.reshape(-1), ctx=ctx), to_gpu(prepared.bin, ctx=ctx)
        d_out = [None if a is None else zeros(a.size, a.dtype, ctx=ctx) for a in out]

        def device():
            _lib.check(ctx._lib.chroma_direction_seed(ctx.handle, ctypes.byref(prepared.struct), ctypes.byref(prepared.timing), vertex_seeder.nchannels,
                                                      p(runner.channel_pos), ncand, p(runner.cand), nfits, _lib.ptr(prepared.offsets), _lib.ptr(prepared.tau0),
                                                      p(d_vertex), p(d_bin), *([p(a) for a in hits] + [p(a) for a in d_out])), ctx._lib)

        device()
        times = clocked(device, ctx.synchronize, args.repeats, args.window)
        got = [None if a is None else d.get().reshape(a.shape) for a, d in zip(out, d_out)]
        fits = seeder.finish(prepared, got)
        # the host twin on the first fits
        nhost = min(nfits, args.host_fits)
        part = seeder.prepare(seeds[0:nhost], offsets[:nhost + 1], channel[:nhost * nhits])
        want = seeder.run_host(part)
        host_times = clocked(lambda: seeder.run_host(part), lambda: None, max(1, args.repeats // 2), args.window)
        same = all(a is None or np.array_equal(a, b[:nhost]) for a, b in zip(want, got))
        evals = float(nhits) * per_hit
        dev, hst = statistics.median(times), statistics.median(host_times) / nhost
        angle = np.degrees(np.arccos(np.clip((fits.dir * axis).sum(axis=1), -1.0, 1.0)))
        print('%5d fits x %5d hits x %5d candidates: device %s = %10.0f fits/s %.3e evaluations/s | host %s for %d fits = %8.1f fits/s %.3e evaluations/s | '
              'x %.1f | first %d fits the same: %s' % (nfits, nhits, ncand, summary(times), nfits / dev, nfits * evals / dev, summary(host_times), nhost, 1.0 / hst,
                                                       evals / hst, hst * nfits / dev, nhost, same))
        print('      angle to the true axis: median %.2f deg, 90%% %.2f deg, worst %.2f deg; hits outside: %.1f %%'
              % (np.median(angle), np.percentile(angle, 90), angle.max(), 100.0 * fits.outside.sum() / max(1, fits.nhits.sum())))
        if not same:
            return 1
    return 0


if __name__ == '__main__':
    sys.exit(main())
