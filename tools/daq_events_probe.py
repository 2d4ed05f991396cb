"""What Simulation.simulate(run_daq=True) costs end to end, by the size of the events of a 1e6-photon batch:

    python tools/daq_events_probe.py [--repeats 5] [--label NAME] [--config EVENTSxPHOTONS ...]

demo.tiny(), isotropic bombs from the origin made here from a seed, one batch per configuration: 1000 events of 1e3 photons,
100 of 1e4, 1 of 1e6.  Each configuration is run once to warm up and then ``--repeats`` times with run_daq=True and with
run_daq=False in turn (keep_hits=False both times); every run ends with the events in hand, so the host clock around it
covers the device work.  Prints per configuration the median and the spread (min .. max) of both, and their difference: what
the DAQ of the batch costs.  Run it on two commits on the same machine, one after the other, to compare them."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

import numpy as np

from chroma_amd import demo
from chroma_amd.event import Photons
from chroma_amd.loader import create_geometry_from_obj
from chroma_amd.sim import Simulation

CONFIGS = [(1000, 1000), (100, 10000), (1, 1000000)]          # (events, photons per event)


def bomb(n, seed):
    rng = np.random.default_rng(seed)

    def sphere():
        phi, u = rng.uniform(0, 2 * np.pi, n), rng.uniform(-1, 1, n)
        c = np.sqrt(1 - u * u)
        return np.column_stack([c * np.cos(phi), c * np.sin(phi), u])
    direction = sphere()
    pol = np.cross(sphere(), direction)
    pol /= np.linalg.norm(pol, axis=1)[:, None]
    return Photons(np.zeros((n, 3)), direction, pol, np.full(n, 400.0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--label', default='')
    ap.add_argument('--config', action='append', help='EVENTSxPHOTONS, e.g. 1x1000000; may be given more than once (default: the three above)')
    args = ap.parse_args()
    sim = Simulation(create_geometry_from_obj(demo.tiny()), seed=5)
    print('# %s  Simulation.simulate(keep_hits=False) on demo.tiny(), one batch, %d repeats after one warm-up; ms, median (min .. max)'
          % (args.label, args.repeats))
    print('# events x photons |        run_daq=True        |        run_daq=False       | difference of the medians | channels hit')
    configs = [tuple(int(float(x)) for x in c.split('x')) for c in args.config] if args.config else CONFIGS
    for nevents, nphotons in configs:
        events = [bomb(nphotons, seed=1000 + k) for k in range(nevents)]
        times = {True: [], False: []}
        nhit = 0
        for repeat in range(args.repeats + 1):
            for run_daq in (True, False):
                t0 = time.perf_counter()
                out = list(sim.simulate(events, run_daq=run_daq, keep_hits=False, photons_per_batch=nevents * nphotons, max_steps=100))
                dt = time.perf_counter() - t0
                assert len(out) == nevents
                if run_daq:
                    nhit = sum(int(ev.channels.hit.sum()) for ev in out)
                if repeat:
                    times[run_daq].append(1e3 * dt)
                out = None
        cell = lambda ts: '%8.1f (%7.1f .. %7.1f)' % (statistics.median(ts), min(ts), max(ts))
        print('%6d x %-8d | %s | %s | %8.1f | %d' % (nevents, nphotons, cell(times[True]), cell(times[False]),
                                                    statistics.median(times[True]) - statistics.median(times[False]), nhit), flush=True)


if __name__ == '__main__':
    main()
