"""What the trigger on the time-binned DAQ of a 1e6-photon batch costs, by the size of its events, beside the pulse acquisition
it follows:

    python tools/daq_trigger_probe.py [--repeats 5] [--label NAME] [--bins 1000] [--trigger 6,8,64,16,48] [--kind nhit] [--config EVENTSxPHOTONS ...]

The inputs of tools/daq_pulses_probe.py: demo.tiny(), isotropic bombs from the origin made here from a seed (1000 events of 1e3
photons, 100 of 1e4, 1 of 1e6), propagated ONCE and left on the device, a window of ``--bins`` bins of 0.25 ns from -8 ns on.
Then, ``--repeats`` times after one warm-up each and interleaved: ``GPUEventDaq.acquire_pulses`` without a trigger (the
yardstick), the same with ``trigger=`` (the pulses triggered on the device before they are read back; the library call inside it,
chroma_daq_trigger_pulses, by the host clock around it -- it returns with its work done), and ``EventPulses.trigger`` on the
fetched pulses (the NumPy twin on the host).  Every one ends with its results on the host, so the host clock covers the device
work.  The share of each kernel inside the call is a kernel trace's to give."""
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
from daq_pulses_probe import Clocked


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--label', default='')
    ap.add_argument('--bins', type=int, default=1000)
    ap.add_argument('--trigger', default='6,8,64,16,48', help='THRESHOLD,WIDTH,HOLDOFF,PRE,POST in bins')
    ap.add_argument('--kind', default='nhit', choices=('nhit', 'npe'))
    ap.add_argument('--config', action='append', help='EVENTSxPHOTONS, e.g. 1x1000000; may be given more than once (default: the three above)')
    args = ap.parse_args()
    sim = Simulation(create_geometry_from_obj(demo.tiny()), seed=5)
    daq = gpu.GPUEventDaq(sim.gpu_geometry)
    lib = sim.context._lib
    call = lib.chroma_daq_trigger_pulses = Clocked(lib.chroma_daq_trigger_pulses)
    window = (-8.0, 0.25, args.bins)
    trigger = gpu.DaqTrigger(*[int(x) for x in args.trigger.split(',')], kind=args.kind)
    print('# %s  GPUEventDaq on demo.tiny(), one propagated batch, window %r, %r, %d repeats after one warm-up; ms, median (min .. max)'
          % (args.label, window, trigger, args.repeats))
    print('# events x photons |   acquire_pulses (yardstick)  | acquire_pulses(trigger=...)    |   of it the trigger call      | '
          'EventPulses.trigger on the host | with / without | pulses | triggers | gated hits | events that fired')
    configs = [tuple(int(float(x)) for x in c.split('x')) for c in args.config] if args.config else CONFIGS
    for nevents, nphotons in configs:
        events = [event.Event(photons_beg=bomb(nphotons, seed=1000 + k)) for k in range(nevents)]
        for k, ev in enumerate(events):
            ev.photons_beg.evidx[:] = k
        gpu_photons, bounds = sim._upload_batch(events, upload=False)
        gpu_photons.propagate(sim.gpu_geometry, sim.rng_states, max_steps=100)
        sim.context.synchronize()
        times = {'plain': [], 'triggered': [], 'call': [], 'host': []}
        for repeat in range(args.repeats + 1):
            t0 = time.perf_counter()
            plain = daq.acquire_pulses(gpu_photons, sim.rng_states, bounds, window, acquisition=0)
            t1 = time.perf_counter()
            call.ms = 0.0
            pulses = daq.acquire_pulses(gpu_photons, sim.rng_states, bounds, window, acquisition=0, trigger=trigger)
            t2 = time.perf_counter()
            twin = plain.trigger(trigger)
            t3 = time.perf_counter()
            if repeat:
                times['plain'].append(1e3 * (t1 - t0))
                times['triggered'].append(1e3 * (t2 - t1))
                times['call'].append(call.ms)
                times['host'].append(1e3 * (t3 - t2))
        t = pulses.triggers
        assert np.array_equal(t.bin, twin.bin) and np.array_equal(t.offsets, twin.offsets) and np.array_equal(t.hit_npe, twin.hit_npe)
        cell = lambda ts: '%8.2f (%7.2f .. %7.2f)' % (statistics.median(ts), min(ts), max(ts))
        print('%6d x %-8d | %s | %s | %s | %s | %5.2f | %d | %d | %d | %d'
              % (nevents, nphotons, cell(times['plain']), cell(times['triggered']), cell(times['call']), cell(times['host']),
                 statistics.median(times['triggered']) / statistics.median(times['plain']), len(pulses.channel), len(t.bin), len(t.hit_channel),
                 int((np.diff(t.offsets) > 0).sum())), flush=True)
        del gpu_photons, plain, pulses, twin


if __name__ == '__main__':
    main()
