#!/usr/bin/env python
"""Both tracking paths on the same photons: GPUPhotons.propagate(track=True) + the per-row regrouping of
Simulation(photon_tracking=True) against GPUPhotons.propagate_tracks, and the tracked library call against the untracked
propagate.  One JSON line per bomb size.  The recorded comparison (profiles/) is the one on the default
geometry, demo.detector(); a smaller builder of chroma_amd.demo is for trying the tool out.

    python tools/track_probe.py [--geometry detector] [--nphotons 100000,1000000] [--max-steps 10] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def regroup(step_ids_list, step_photons_list, n):
    """The loop of Simulation._simulate_batch (chroma_amd.tracks.host_tracks) for one event of ``n`` photons."""
    from chroma_amd import event
    tracks = [[] for _ in range(n)]
    for step_ids, step_photons in zip(step_ids_list, step_photons_list):
        for k, pid in enumerate(step_ids):
            tracks[pid].append(step_photons[k])
    return [event.Photons.join(t, concatenate=False) if len(t) > 0 else event.Photons() for t in tracks]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--geometry', default='detector', help='a builder of chroma_amd.demo')
    ap.add_argument('--nphotons', default='100000,1000000')
    ap.add_argument('--max-steps', type=int, default=10)
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--out', default=None, help='also append the JSON lines to this file')
    args = ap.parse_args(argv)

    from chroma_amd import demo, gpu, _lib
    from chroma_amd.loader import create_geometry_from_obj
    from chroma_amd.gpu.geometry import pack_geometry
    from chroma_amd.gpu.photon import generate_bomb, _structure

    ctx = gpu.create_cuda_context(0)
    t0 = time.time()
    packed = pack_geometry(create_geometry_from_obj(getattr(demo, args.geometry)())).attach_wide_tree()
    gg = gpu.GPUDetector.from_packed(packed)
    print('%s: %d triangles in %.1f s' % (args.geometry, packed.desc.ntriangles, time.time() - t0), file=sys.stderr, flush=True)

    def photons(n):
        return generate_bomb(n, args.seed, wavelength_lo=400.0)

    def timed(fn):
        ctx.synchronize()
        t = time.time()
        out = fn()
        ctx.synchronize()
        return out, time.time() - t

    def library_call(gp, tracked):
        """Wall time of the library call alone (it returns when the photons, and the rows, are complete)."""
        s = _structure(gp)
        opt = _lib.PropagateOptions(args.max_steps, tail=1 if tracked else -1)
        rng = _lib.Rng(12345, 0)
        st, aborted = _lib.PropagateStats(), ctypes.c_int32(0)
        handle, nrows = ctypes.c_void_p(), ctypes.c_uint64(0)

        def call():
            if tracked:
                _lib.check(ctx._lib.chroma_propagate_tracks(ctx.handle, gg.handle, ctypes.byref(s), len(gp), 1, rng, ctypes.byref(opt),
                                                            ctypes.byref(st), ctypes.byref(aborted), ctypes.byref(handle), ctypes.byref(nrows)))
            else:
                _lib.check(ctx._lib.chroma_propagate_opt(ctx.handle, gg.handle, ctypes.byref(s), len(gp), 1, rng, ctypes.byref(opt),
                                                         ctypes.byref(st), ctypes.byref(aborted), None))
        _, dt = timed(call)
        if tracked:
            _lib.check(ctx._lib.chroma_tracks_destroy(ctx.handle, handle))
        return dt, int(nrows.value)

    rng_states = _lib.Rng(12345, 0)
    # (first calls allocate the context's queues and fill the pool: not timed)
    photons(1000).propagate_tracks(gg, rng_states, max_steps=args.max_steps)
    photons(1000).propagate(gg, rng_states, max_steps=args.max_steps, track=True)
    for n in [int(float(x)) for x in args.nphotons.split(',')]:
        row = {'geometry': args.geometry, 'nphotons': n, 'max_steps': args.max_steps}
        library_call(photons(n), True)                                  # (the pool gets this size's slabs)
        row['untracked_call_s'], _ = library_call(photons(n), False)
        row['tracked_call_s'], nrows = library_call(photons(n), True)
        row['rows'], row['row_bytes'] = nrows, 64 * nrows
        tracks, row['propagate_tracks_s'] = timed(lambda: photons(n).propagate_tracks(gg, rng_states, max_steps=args.max_steps))
        print('%d photons: device path done' % n, file=sys.stderr, flush=True)
        (ids, steps), row['track_true_s'] = timed(lambda: photons(n).propagate(gg, rng_states, max_steps=args.max_steps, track=True))
        print('%d photons: propagate(track=True) done, regrouping' % n, file=sys.stderr, flush=True)
        t = time.time()
        grouped = regroup(ids, steps, n)
        row['regroup_s'] = time.time() - t
        row['track_true_total_s'] = row['track_true_s'] + row['regroup_s']
        assert len(grouped) == len(tracks) and sum(len(g) for g in grouped) == nrows == len(tracks.photons)
        row['speedup_end_to_end'] = row['track_true_total_s'] / row['propagate_tracks_s']
        line = json.dumps({k: (round(v, 5) if isinstance(v, float) else v) for k, v in row.items()})
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, 'a') as f:
                f.write(line + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
