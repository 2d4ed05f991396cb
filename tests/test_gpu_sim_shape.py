"""Simulation.simulate() end to end on the tiny detector, every path of it, against digests of what the commit before its host side
was taken apart (cb01f9e) hung on the events: photons in with hits and end photons; the same through the whole readout chain,
with and without the traces; events with steps through the chain up to the trigger; bare vertices through the stepper; and
both kinds of photon tracks.  A digest is a SHA-256 over every array and number on every event, fields in name order, an
event's hits first sorted over all their columns (the order of hits within a channel is the device's).

tests/golden/sim_shape_digests.json holds the digests and the commit they were recorded on (twice, with equal results)."""
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, bomb

pytestmark = pytest.mark.gpu

SEED = 4711
SIZES = [500, 1200, 3000, 800, 6000, 700, 2500, 900, 5200]          # at 5000 a batch: four events, one, four
PER_BATCH = 5000
WINDOW = (-8.0, 0.5, 512)
PHOTONS_PER_MM = 94.45          # what a segment at beta = 1 emits at most in the tiny detector's brightest medium, about
PHOTONS_PER_MEV = 493.4         # what an electron's kinetic energy is worth in the stepper's bound, about


# ---- the digest --------------------------------------------------------------------------------------------------------
def sorted_hits(hits):
    """``hits`` (a Photons) in the order of a lexsort over all its columns, as bits."""
    from chroma_amd.event import _PHOTON_FIELDS
    columns = [np.ascontiguousarray(getattr(hits, name)).view(np.uint32).reshape(len(hits), -1) for name in _PHOTON_FIELDS]
    return hits[np.lexsort(np.concatenate(columns, axis=1).T[::-1])]


def walk(value, path, out, seen):
    """Every array and plain value below ``value`` as (path, bytes) into ``out``: attributes and keys in sorted order, objects of
    the package by their attributes, what lives on the device and anything foreign by its type's name alone."""
    if isinstance(value, np.ndarray):
        out.append((path, ('%s%s' % (value.dtype.str, value.shape)).encode() + np.ascontiguousarray(value).tobytes()))
    elif value is None or isinstance(value, (bool, int, float, str, bytes, np.generic)):
        out.append((path, repr(value.item() if isinstance(value, np.generic) else value).encode()))
    elif isinstance(value, (list, tuple)):
        out.append((path, ('%d items' % len(value)).encode()))
        for k, item in enumerate(value):
            walk(item, '%s[%d]' % (path, k), out, seen)
    elif isinstance(value, dict):
        out.append((path, ('%d keys' % len(value)).encode()))
        for key in sorted(value):
            walk(value[key], '%s[%r]' % (path, key), out, seen)
    elif type(value).__module__.startswith('chroma_amd') and hasattr(value, '__dict__') and 'gpu.tools' not in type(value).__module__:
        if id(value) in seen:
            out.append((path, b'seen ' + seen[id(value)][0].encode()))
            return
        seen[id(value)] = (path, value)          # (held: a sorted copy's id is not handed out again while the walk lasts)
        for name in sorted(vars(value)):
            item = vars(value)[name]
            if type(value).__name__ == 'Event' and item is not None and name in ('flat_hits', 'hits'):
                item = sorted_hits(item) if name == 'flat_hits' else {c: sorted_hits(h) for c, h in item.items()}
            walk(item, '%s.%s' % (path, name), out, seen)
    else:
        out.append((path, ('a %s' % type(value).__name__).encode()))


def fields(events):
    out = []
    seen = {}          # (one per scenario: the settings and seeders the events share are walked once)
    for k, ev in enumerate(events):
        walk(ev, 'ev%d' % k, out, seen)
    return out


def digest(events, leave_out=()):
    h = hashlib.sha256()
    for path, data in fields(events):
        if not any(part in path for part in leave_out):
            h.update(path.encode() + b'\0' + hashlib.sha256(data).digest())
    return h.hexdigest()


# ---- the scenarios -----------------------------------------------------------------------------------------------------
def photon_events(sizes=SIZES):
    return [bomb(n, seed=900 + k) for k, n in enumerate(sizes)]


def chain(gpu, geometry):
    from chroma_amd.seed import VertexSeeder
    digitizer = gpu.DaqDigitizer.biexponential(30.0, 1.0, 6.0, 0.5, bits=12, pedestal=150, noise_sigma=2.0)
    return dict(run_daq=True, daq_window=WINDOW, daq_trigger=gpu.DaqTrigger(2, 16, 64, 8, 40), daq_noise=2000.0, daq_digitizer=digitizer,
                daq_reducer=gpu.DaqReducer.for_digitizer(digitizer, 8, lead=2, lag=6, nbaseline=4, min_width=2, time_offset_ns=0.75),
                daq_seeder=VertexSeeder.for_detector(geometry, 200.0, levels=3, weights='npe'), daq_direction=(0.75, 0.2, 0.1, 2))


def stepped_events():
    """Events whose one vertex carries the steps of a fast muon-like track: event k emits about SIZES[k] photons at most"""
    from chroma_amd import event
    events = []
    for k, size in enumerate(SIZES):
        nseg, start = 3 + k % 4, (-50.0 + 10.0 * k, 3.0 * k, -7.0)
        length = size / PHOTONS_PER_MM
        n = nseg + 1
        x = start[0] + np.linspace(0.0, length, n)
        dep = np.concatenate(([0.0], np.full(nseg, 0.2 * length / nseg)))
        steps = event.Steps(x, np.full(n, start[1]), np.full(n, start[2]), (x - x[0]) / 299.79, np.ones(n), np.zeros(n), np.zeros(n),
                            4000.0 - np.cumsum(dep), dep, dep)
        events.append(event.Event(vertices=[event.Vertex('mu-', start, (1, 0, 0), 4000.0, steps=steps, pdgcode=13)]))
    return events


def electrons():
    """Bare vertices: electron k is worth about SIZES[k] photons in the stepper's bound"""
    from chroma_amd import event
    rng = np.random.default_rng(SEED)
    out = []
    for size in SIZES:
        direction = rng.normal(size=3)
        out.append(event.Vertex('e-', tuple(rng.uniform(-300.0, 300.0, 3)), tuple(direction / np.linalg.norm(direction)), size / PHOTONS_PER_MEV, pdgcode=11))
    return out


def run(name, gpu, geometry):
    """The events of scenario ``name``, each on a Simulation of its own."""
    from chroma_amd.sim import Simulation
    common = dict(photons_per_batch=PER_BATCH, max_steps=100)
    if name == 'photons':
        return list(Simulation(geometry, seed=SEED).simulate(photon_events(), keep_photons_end=True, **common))
    if name in ('chain', 'chain_without_traces'):
        return list(Simulation(geometry, seed=SEED).simulate(photon_events(), keep_photons_end=True, daq_keep_traces=name == 'chain',
                                                            **dict(common, **chain(gpu, geometry))))
    if name == 'stepped':
        return list(Simulation(geometry, seed=SEED, light_medium='located').simulate(stepped_events(), run_daq=True, daq_window=WINDOW,
                                                                                    daq_trigger=(2, 16, 64, 8, 40), **common))
    if name == 'tracked':
        return list(Simulation(geometry, seed=SEED, stepper='csda').simulate(electrons(), **common))
    tracking = {'host_tracks': True, 'device_tracks': 'device'}[name]
    return list(Simulation(geometry, seed=SEED, photon_tracking=tracking).simulate(photon_events([300, 300]), photons_per_batch=1000, max_steps=100))


SCENARIOS = ('photons', 'chain', 'chain_without_traces', 'stepped', 'tracked', 'host_tracks', 'device_tracks')


@pytest.fixture(scope='module')
def gpu():
    from chroma_amd import gpu as g
    ctx = g.create_cuda_context(0)
    yield g
    ctx.pop()


@pytest.fixture(scope='module')
def recorded():
    with open(os.path.join(GOLDEN, 'sim_shape_digests.json')) as f:
        return json.load(f)


@pytest.mark.parametrize('name', SCENARIOS)
def test_simulate_hangs_on_the_events_what_it_did_before(gpu, tiny_geometry, recorded, name):
    events = run(name, gpu, tiny_geometry)
    assert [ev.id for ev in events] == list(range(2 if 'tracks' in name else len(SIZES)))
    assert all(ev.nphotons > 0 for ev in events)
    if name.startswith('chain'):
        assert sum(len(ev.triggers) for ev in events) >= 5 and all(len(ev.triggers.vertices) == len(ev.triggers.directions) == len(ev.triggers) for ev in events)
    assert digest(events, recorded['left_out']) == recorded['digests'][name]
