"""What the time-binned DAQ of a 1e6-photon batch costs, by the size of its events, beside the batch DAQ it is a second view of:

    python tools/daq_pulses_probe.py [--repeats 5] [--label NAME] [--bins 1000] [--config EVENTSxPHOTONS ...]

demo.tiny(), isotropic bombs from the origin made here from a seed (the batches of tools/daq_events_probe.py: 1000 events of
1e3 photons, 100 of 1e4, 1 of 1e6), propagated ONCE and left on the device.  Then, on those photons, ``--repeats`` times after
one warm-up each: ``GPUEventDaq.acquire`` (the yardstick: per (event, channel), it does less work) and
``GPUEventDaq.acquire_pulses`` with a window of ``--bins`` bins of 0.25 ns from -8 ns on.  Both end with their results on the
host, so the host clock around them covers the device work.  The pulses' time is split by the clock around its two library
calls: the count (chroma_daq_count_pulses), the acquisition (chroma_daq_acquire_pulses: count again, emit, sort, reduce) and the
rest (buffers and read-back).  The share of each kernel inside the acquisition is a kernel trace's to give."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

import numpy as np

from chroma_amd import demo, event
from chroma_amd.loader import create_geometry_from_obj
from chroma_amd.sim import Simulation
from chroma_amd import gpu

from daq_events_probe import CONFIGS, bomb


class Clocked(object):
    """A library call with the host clock around it (every one of the two returns with its work done)."""

    def __init__(self, fn):
        self.fn, self.ms = fn, 0.0

    def __call__(self, *args):
        t0 = time.perf_counter()
        rc = self.fn(*args)
        self.ms += 1e3 * (time.perf_counter() - t0)
        return rc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--label', default='')
    ap.add_argument('--bins', type=int, default=1000)
    ap.add_argument('--config', action='append', help='EVENTSxPHOTONS, e.g. 1x1000000; may be given more than once (default: the three above)')
    args = ap.parse_args()
    sim = Simulation(create_geometry_from_obj(demo.tiny()), seed=5)
    daq = gpu.GPUEventDaq(sim.gpu_geometry)
    lib = sim.context._lib
    count = lib.chroma_daq_count_pulses = Clocked(lib.chroma_daq_count_pulses)
    acquire = lib.chroma_daq_acquire_pulses = Clocked(lib.chroma_daq_acquire_pulses)
    window = (-8.0, 0.25, args.bins)
    print('# %s  GPUEventDaq on demo.tiny(), one propagated batch, window %r, %d repeats after one warm-up; ms, median (min .. max)'
          % (args.label, window, args.repeats))
    print('# events x photons |      acquire (yardstick)      |         acquire_pulses        | count call | acquire call | rest | '
          'channels hit | pulses | accepted in window | outside')
    configs = [tuple(int(float(x)) for x in c.split('x')) for c in args.config] if args.config else CONFIGS
    for nevents, nphotons in configs:
        events = [event.Event(photons_beg=bomb(nphotons, seed=1000 + k)) for k in range(nevents)]
        for k, ev in enumerate(events):
            ev.photons_beg.evidx[:] = k
        gpu_photons, bounds = sim._upload_batch(events, upload=False)
        gpu_photons.propagate(sim.gpu_geometry, sim.rng_states, max_steps=100)
        sim.context.synchronize()
        times = {'acquire': [], 'pulses': [], 'count': [], 'call': []}
        for repeat in range(args.repeats + 1):
            t0 = time.perf_counter()
            channels = daq.acquire(gpu_photons, sim.rng_states, bounds, acquisition=0)
            t1 = time.perf_counter()
            count.ms = acquire.ms = 0.0
            pulses = daq.acquire_pulses(gpu_photons, sim.rng_states, bounds, window, acquisition=0)
            t2 = time.perf_counter()
            if repeat:
                times['acquire'].append(1e3 * (t1 - t0))
                times['pulses'].append(1e3 * (t2 - t1))
                times['count'].append(count.ms)
                times['call'].append(acquire.ms)
        nhit = sum(len(channels.sparse(i)[0]) for i in range(nevents))
        outside = sum(sum(pulses.outside(i)) for i in range(nevents))
        cell = lambda ts: '%8.2f (%7.2f .. %7.2f)' % (statistics.median(ts), min(ts), max(ts))
        med = {k: statistics.median(v) for k, v in times.items()}
        print('%6d x %-8d | %s | %s | %8.2f | %8.2f | %8.2f | %d | %d | %d | %d'
              % (nevents, nphotons, cell(times['acquire']), cell(times['pulses']), med['count'], med['call'],
                 med['pulses'] - med['count'] - med['call'], nhit, len(pulses.channel), int(pulses.npe.sum(dtype=np.uint64)), outside), flush=True)
        del gpu_photons, channels, pulses


if __name__ == '__main__':
    main()
