"""``chroma-sim``: run photon-bomb events through a detector and write the hits.

The reference driver (bin/chroma-sim:32-112) takes a detector string, generates events with
GEANT4 and writes a ROOT file; neither GEANT4 nor ROOT is part of this engine, so this driver
keeps the command-line shape (detector string, -n/--nevents, -o/--output, -s/--seed, -j device)
but the particle source is the isotropic photon bomb of chroma/benchmark.py:77-83 and the output is
an ``.npz``: per event the flat hits (channel, t, wavelength, pos, flags), with --run-daq the channel
times and charges, with --daq-window T0,DT,NBINS also the pulses per (channel, time bin), with --daq-trigger the triggers on them, with --daq-digitize the ADC traces of their gates, with --daq-reduce the pulses found in the traces, with --daq-noise RATE_HZ dark noise among them, with --save-photons-beg/--save-photons-end the photons themselves and with --track or
--device-tracks every photon's state after each step.
"""
import argparse
import sys
import time

import numpy as np


def bomb_event(nphotons, wavelength, pos, rng):
    from chroma_amd.event import Photons
    theta = rng.uniform(0, 2 * np.pi, nphotons)
    u = rng.uniform(-1, 1, nphotons)
    c = np.sqrt(1 - u * u)
    d = np.column_stack([c * np.cos(theta), c * np.sin(theta), u])
    theta = rng.uniform(0, 2 * np.pi, nphotons)
    u = rng.uniform(-1, 1, nphotons)
    c = np.sqrt(1 - u * u)
    a = np.column_stack([c * np.cos(theta), c * np.sin(theta), u])
    pol = np.cross(a, d)
    pol /= np.linalg.norm(pol, axis=1)[:, None]
    if isinstance(wavelength, tuple):
        wl = rng.uniform(wavelength[0], wavelength[1], nphotons)
    else:
        wl = np.full(nphotons, wavelength)
    return Photons(np.tile(np.asarray(pos, dtype=float), (nphotons, 1)), d, pol, wl)


def main(argv=None):
    ap = argparse.ArgumentParser(prog='chroma-sim', description=__doc__.split('\n\n')[0])
    ap.add_argument('detector', help='"@module.function" returning a Detector/Geometry, e.g. @chroma_amd.demo.tiny')
    ap.add_argument('-o', '--output', default='out.npz')
    ap.add_argument('-n', '--nevents', type=int, default=10)
    ap.add_argument('-s', '--seed', type=int, default=None)
    ap.add_argument('-j', '--device', type=int, default=None, help='GPU index')
    ap.add_argument('--nphotons', type=int, default=100000, help='photons per event')
    ap.add_argument('--wavelength', default='400', help='nm, or "lo:hi" for a uniform range')
    ap.add_argument('--pos', default='0,0,0')
    ap.add_argument('--particle', default=None, metavar='NAME',
                    help='instead of a photon bomb: one charged particle per event at --pos (e-, e+, mu-, mu+, pi+, pi-, K+, K-, p, alpha), '
                         'stepped through the detector on the GPU (continuous slowing down, no secondaries: Simulation(stepper=\'csda\'))')
    ap.add_argument('--ke', type=float, default=None, metavar='MEV', help='with --particle: its kinetic energy')
    ap.add_argument('--dir', default='0,0,1', metavar='X,Y,Z', help='with --particle: its direction')
    ap.add_argument('--save-steps', action='store_true', help='with --particle: also write the step points of every event')
    ap.add_argument('--max-steps', type=int, default=100)
    ap.add_argument('--run-daq', action='store_true')
    ap.add_argument('--daq-window', default=None, metavar='T0,DT,NBINS',
                    help='also write the time-binned DAQ: the pulses per (channel, bin) of NBINS bins of DT ns from T0 on (implies --run-daq)')
    ap.add_argument('--daq-trigger', default=None, metavar='THRESHOLD,WIDTH[,HOLDOFF,PRE,POST]',
                    help='with --daq-window, also write the triggers on the pulses: the firings of a sum over WIDTH bins that reaches THRESHOLD, '
                         'HOLDOFF bins apart at the least, and the channels in each gate of PRE bins before to POST bins from the firing')
    ap.add_argument('--daq-trigger-kind', default='nhit', choices=('nhit', 'npe'), help='what the trigger sums: distinct channels or photoelectrons')
    ap.add_argument('--daq-noise', default=None, type=float, metavar='RATE_HZ',
                    help='with --daq-window, add PMT dark noise of RATE_HZ per channel to the pulses (and to what the trigger sees)')
    ap.add_argument('--daq-digitize', default=None, metavar='AMPLITUDE,RISE_NS,FALL_NS[,BITS[,PEDESTAL[,SIGMA]]]',
                    help='with --daq-trigger, also write the ADC trace of every channel in every gate: a biexponential pulse of AMPLITUDE counts per '
                         'unit charge, read with BITS bits on PEDESTAL counts and electronics noise of SIGMA counts')
    ap.add_argument('--daq-reduce', default=None, metavar='THRESHOLD[,LEAD,LAG[,CFD[,NBASELINE[,MIN_WIDTH]]]]',
                    help='with --daq-digitize, also write the pulses found in the traces (trigger_found_*, trigger_trace_base): runs of MIN_WIDTH samples '
                         'THRESHOLD counts above the baseline (the digitiser\'s pedestal, or the mean of the first NBASELINE samples), integrated from LEAD '
                         'samples before to LAG behind, timed at the fraction CFD of the peak')
    ap.add_argument('--daq-seed', default=None, metavar='SPEED_MM_PER_NS[,SPACING_MM[,LEVELS]]',
                    help='with --daq-trigger, also write a seed vertex per firing (seed_pos in mm, seed_t0 in ns, seed_score, seed_outside): the '
                         'position and time at which the time residuals of the firing pile up best for light at SPEED_MM_PER_NS, searched on a '
                         'grid of SPACING_MM (default: the detector radius / 8) and refined on LEVELS shrinking lattices (default 6); from the '
                         'found pulses with --daq-reduce, else from the truth-level hits of the gate')
    ap.add_argument('--daq-direction', default=None, metavar='COS_C[,SIGMA_COS[,FILL[,LEVELS]]]',
                    help='with --daq-seed, also write a seed direction per firing (dir_dir, dir_score, dir_inside, dir_outside, dir_level_score): '
                         'the axis about which the firing\'s hits, seen from the seed vertex, best fill a cone of cosine COS_C -- a Gaussian '
                         'profile of SIGMA_COS (default 0.1), FILL (0 .. 1) of its peak inside the cone (default 0) -- searched on a grid of 864 '
                         'directions and refined on LEVELS shrinking lattices (default 6)')
    ap.add_argument('--daq-drop-traces', action='store_true', help='with --daq-reduce, do not read the traces back: trigger_adc is not written')
    ap.add_argument('--save-photons-beg', action='store_true', help='also write the initial photons of every event (bin/chroma-sim:51-53)')
    ap.add_argument('--save-photons-end', action='store_true', help='also write the final photons of every event (bin/chroma-sim:54-56)')
    ap.add_argument('--track', action='store_true', help='also write every photon\'s state after each step (Simulation(photon_tracking=True))')
    ap.add_argument('--device-tracks', action='store_true', help='what --track writes, recorded on the device (Simulation(photon_tracking=\'device\'))')
    ap.add_argument('--exact', action='store_true', help='the reference\'s own traversal loop for every ray: its hit triangle on EVERY ray, several times slower (Simulation(exact=True))')
    ap.add_argument('--cache-dir', default=None, help='directory of the BVH cache (off by default)')
    args = ap.parse_args(argv)

    from chroma_amd.loader import load_geometry_from_string
    from chroma_amd.sim import Simulation

    wl = tuple(float(x) for x in args.wavelength.split(':')) if ':' in args.wavelength else float(args.wavelength)
    pos = [float(x) for x in args.pos.split(',')]
    if args.particle is not None:
        from chroma_amd.generator.particles import PDG_CODES
        if args.particle not in PDG_CODES:
            ap.error('--particle: one of %s' % ', '.join(sorted(PDG_CODES)))
        if args.ke is None or not args.ke > 0:
            ap.error('--particle needs --ke MEV above 0')
        direction = [float(x) for x in args.dir.split(',')]
        if len(direction) != 3 or not any(direction):
            ap.error('--dir takes X,Y,Z, not all zero')
        if args.track or args.device_tracks:
            ap.error('--particle does not go with --track or --device-tracks')
    elif args.ke is not None or args.save_steps:
        ap.error('--ke and --save-steps need --particle')
    daq_window = None
    if args.daq_window is not None:
        parts = args.daq_window.split(',')
        if len(parts) != 3:
            ap.error('--daq-window takes T0,DT,NBINS')
        daq_window = (float(parts[0]), float(parts[1]), int(parts[2]))
        args.run_daq = True
    daq_trigger = None
    if args.daq_trigger is not None:
        if daq_window is None:
            ap.error('--daq-trigger needs --daq-window')
        parts = args.daq_trigger.split(',')
        if len(parts) not in (2, 5):
            ap.error('--daq-trigger takes THRESHOLD,WIDTH[,HOLDOFF,PRE,POST]')
        from chroma_amd.gpu.daq import DaqTrigger
        try:
            daq_trigger = DaqTrigger(*[int(x) for x in parts], kind=args.daq_trigger_kind)
        except ValueError as e:
            ap.error('--daq-trigger: %s' % e)
    if args.daq_noise is not None:
        if daq_window is None:
            ap.error('--daq-noise needs --daq-window')
        if not (args.daq_noise >= 0.0 and args.daq_noise < float('inf')):
            ap.error('--daq-noise takes a finite rate that is not negative')
    daq_digitizer = None
    if args.daq_digitize is not None:
        if daq_trigger is None:
            ap.error('--daq-digitize needs --daq-trigger')
        parts = args.daq_digitize.split(',')
        if not 3 <= len(parts) <= 6:
            ap.error('--daq-digitize takes AMPLITUDE,RISE_NS,FALL_NS[,BITS[,PEDESTAL[,SIGMA]]]')
        from chroma_amd.gpu.daq import DaqDigitizer
        try:
            kw = dict(bits=int(parts[3]) if len(parts) > 3 else 14, pedestal=int(parts[4]) if len(parts) > 4 else 0,
                      noise_sigma=float(parts[5]) if len(parts) > 5 else 0.0)
            daq_digitizer = DaqDigitizer.biexponential(float(parts[0]), float(parts[1]), float(parts[2]), daq_window[1], **kw).check(daq_trigger)
        except ValueError as e:
            ap.error('--daq-digitize: %s' % e)
    daq_reducer = None
    if args.daq_reduce is not None:
        if daq_digitizer is None:
            ap.error('--daq-reduce needs --daq-digitize')
        parts = args.daq_reduce.split(',')
        if len(parts) not in (1, 3, 4, 5, 6):
            ap.error('--daq-reduce takes THRESHOLD[,LEAD,LAG[,CFD[,NBASELINE[,MIN_WIDTH]]]]')
        from chroma_amd.gpu.daq import DaqReducer
        try:
            kw = dict(zip(('lead', 'lag', 'cfd', 'nbaseline', 'min_width'), [float(x) if k == 2 else int(x) for k, x in enumerate(parts[1:])]))
            daq_reducer = DaqReducer.for_digitizer(daq_digitizer, int(parts[0]), **kw).check(daq_trigger.pre + daq_trigger.post)
        except ValueError as e:
            ap.error('--daq-reduce: %s' % e)
    elif args.daq_drop_traces:
        ap.error('--daq-drop-traces needs --daq-reduce')
    daq_seeder = None
    if args.daq_seed is not None:
        if daq_trigger is None:
            ap.error('--daq-seed needs --daq-trigger')
        parts = args.daq_seed.split(',')
        try:
            daq_seeder = tuple([float(x) for x in parts[:2]] + [int(x) for x in parts[2:]])
            if not 1 <= len(parts) <= 3 or not daq_seeder[0] > 0:
                raise ValueError('a positive speed')
        except ValueError:
            ap.error('--daq-seed takes SPEED_MM_PER_NS[,SPACING_MM[,LEVELS]]')
    daq_direction = None
    if args.daq_direction is not None:
        if daq_seeder is None:
            ap.error('--daq-direction needs --daq-seed')
        parts = args.daq_direction.split(',')
        try:
            daq_direction = tuple([float(x) for x in parts[:3]] + [int(x) for x in parts[3:]])
            if not 1 <= len(parts) <= 4 or not -1.0 <= daq_direction[0] <= 1.0:
                raise ValueError('a cosine')
        except ValueError:
            ap.error('--daq-direction takes COS_C[,SIGMA_COS[,FILL[,LEVELS]]]')
    t0 = time.time()
    detector = load_geometry_from_string(args.detector, cache_dir=args.cache_dir)
    print('geometry: %d triangles, BVH %d nodes (%.1f s)' % (len(detector.mesh.triangles), len(detector.bvh.nodes), time.time() - t0))
    sim = Simulation(detector, seed=args.seed, cuda_device=args.device, geant4_processes=0,
                     photon_tracking='device' if args.device_tracks else args.track, exact=args.exact,
                     stepper='csda' if args.particle is not None else None, particle_tracking=args.save_steps)
    rng = np.random.default_rng(sim.seed)
    if args.particle is not None:
        from chroma_amd import event
        events = (event.Event(vertices=[event.Vertex(args.particle, pos, direction, args.ke, pdgcode=PDG_CODES[args.particle])])
                  for _ in range(args.nevents))
    else:
        events = (bomb_event(args.nphotons, wl, pos, rng) for _ in range(args.nevents))
    out = {'nevents': np.array(args.nevents), 'nphotons': np.array(args.nphotons), 'seed': np.array(sim.seed)}
    t0 = time.time()
    nhits = nphotons = 0
    for ev in sim.simulate(events, keep_photons_beg=args.save_photons_beg, keep_photons_end=args.save_photons_end,
                           keep_hits=False, keep_flat_hits=hasattr(detector, 'num_channels'),
                           run_daq=args.run_daq, max_steps=args.max_steps, daq_window=daq_window, daq_trigger=daq_trigger,
                           daq_noise=args.daq_noise, daq_digitizer=daq_digitizer, daq_reducer=daq_reducer,
                           daq_keep_traces=not args.daq_drop_traces, daq_seeder=daq_seeder, daq_direction=daq_direction):
        key = 'ev%d' % ev.id
        nphotons += ev.nphotons
        if args.particle is not None:
            out[key + '/nphotons'] = np.array(ev.nphotons)          # (what the particle's track emitted: --nphotons is not used)
        for tag, ph in (('photons_beg', ev.photons_beg), ('photons_end', ev.photons_end)):
            if ph is not None:
                for name in ('pos', 'dir', 'pol', 'wavelengths', 't', 'flags', 'last_hit_triangles', 'weights'):
                    out['%s/%s/%s' % (key, tag, name)] = getattr(ph, name)
        if args.save_steps:
            steps = ev.vertices[0].steps
            for name in ('x', 'y', 'z', 't', 'dx', 'dy', 'dz', 'ke', 'edep', 'qedep'):
                out['%s/steps/%s' % (key, name)] = getattr(steps, name)
        if args.device_tracks and getattr(ev, 'photon_tracks', None) is not None:
            # the same keys straight from the flat rows (PhotonTracks)
            tracks = ev.photon_tracks
            out[key + '/track/photon'] = np.repeat(np.arange(len(tracks), dtype=np.uint32), tracks.steps_taken + 1)
            for name in ('pos', 'dir', 't', 'flags'):
                out['%s/track/%s' % (key, name)] = getattr(tracks.photons, name)
        elif args.track and getattr(ev, 'photon_tracks', None) is not None:
            # one row per (photon, step): ragged tracks flattened, with the photon index beside them
            tracks = ev.photon_tracks
            out[key + '/track/photon'] = np.concatenate([np.full(len(tr), i, dtype=np.uint32) for i, tr in enumerate(tracks)]
                                                         ) if tracks else np.empty(0, dtype=np.uint32)
            for name in ('pos', 'dir', 't', 'flags'):
                parts = [getattr(tr, name) for tr in tracks if len(tr)]
                out['%s/track/%s' % (key, name)] = np.concatenate(parts) if parts else np.empty(0)
        if ev.flat_hits is not None:
            h = ev.flat_hits
            nhits += len(h)
            out[key + '/channel'] = h.channel
            out[key + '/t'] = h.t
            out[key + '/wavelength'] = h.wavelengths
            out[key + '/pos'] = h.pos
            out[key + '/flags'] = h.flags
        if ev.channels is not None:
            out[key + '/daq_hit'] = ev.channels.hit
            out[key + '/daq_t'] = ev.channels.t
            out[key + '/daq_q'] = ev.channels.q
        if ev.pulses is not None:
            out[key + '/pulse_channel'] = ev.pulses.channel
            out[key + '/pulse_bin'] = ev.pulses.bin
            out[key + '/pulse_npe'] = ev.pulses.npe
            out[key + '/pulse_q'] = ev.pulses.q
            out[key + '/pulse_t'] = ev.pulses.t_first
            out[key + '/pulse_outside'] = np.array([ev.pulses.early, ev.pulses.late], dtype=np.uint32)
            if args.daq_noise is not None:
                out[key + '/pulse_flags'] = ev.pulses.flags
                out[key + '/pulse_noise'] = np.array(ev.pulses.noise, dtype=np.uint32)
        if ev.triggers is not None:
            out[key + '/trigger_bin'] = ev.triggers.bin
            out[key + '/trigger_time'] = ev.triggers.time
            out[key + '/trigger_sum'] = ev.triggers.sum
            out[key + '/trigger_hit_offsets'] = ev.triggers.hit_offsets
            out[key + '/trigger_hit_channel'] = ev.triggers.hit_channel
            out[key + '/trigger_hit_npe'] = ev.triggers.hit_npe
            out[key + '/trigger_hit_q'] = ev.triggers.hit_q
            out[key + '/trigger_hit_t'] = ev.triggers.hit_t_first
            out[key + '/pulse_trigger'] = ev.triggers.pulse_trigger
            if ev.triggers.vertices is not None:
                out[key + '/seed_pos'] = ev.triggers.vertices.pos
                out[key + '/seed_t0'] = ev.triggers.vertices.t0
                out[key + '/seed_score'] = ev.triggers.vertices.score
                out[key + '/seed_outside'] = ev.triggers.vertices.outside
            if ev.triggers.directions is not None:
                out[key + '/dir_dir'] = ev.triggers.directions.dir
                out[key + '/dir_score'] = ev.triggers.directions.score
                out[key + '/dir_inside'] = ev.triggers.directions.inside
                out[key + '/dir_outside'] = ev.triggers.directions.outside
                out[key + '/dir_level_score'] = ev.triggers.directions.level_score
            if ev.triggers.traces is not None:
                out[key + '/trigger_adc'] = ev.triggers.traces
            if ev.triggers.trace_flags is not None:
                out[key + '/trigger_trace_flags'] = ev.triggers.trace_flags
            if ev.triggers.reducer is not None:
                from chroma_amd.gpu.daq import FOUND_COLUMNS
                out[key + '/trigger_found_offsets'] = ev.triggers.found_offsets
                for name, _ in FOUND_COLUMNS:
                    out['%s/trigger_%s' % (key, name)] = getattr(ev.triggers, name)
                out[key + '/trigger_trace_base'] = ev.triggers.trace_base
                out[key + '/trigger_reduced_flags'] = ev.triggers.reduced_flags
    dt = time.time() - t0
    np.savez_compressed(args.output, **out)
    print('%d events, %d photons, %d hits in %.2f s (%.1f events/s, %.3g photons/s) -> %s' % (
        args.nevents, nphotons, nhits, dt, args.nevents / dt, nphotons / dt, args.output))
    return 0


if __name__ == '__main__':
    sys.exit(main())
