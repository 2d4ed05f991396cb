"""The host side of Simulation.simulate() after its parts were named, without a GPU: the refusals of simulate() and of
GPUEventDaq.acquire_pulses() word for word as they were, the one batch cutter against the loop it replaced, and the two pure
pieces that left _simulate_batch (the per-channel slices of an event's hits, the host-side track assembly) against the lines
they were."""
import itertools

import numpy as np
import pytest

from chroma_amd import event
from chroma_amd.gpu.daq import DAQ_NEEDS, DaqChain, DaqDigitizer, DaqReducer, DaqTrigger, GPUEventDaq
from chroma_amd.sim import Simulation, cut_batches, hits_by_channel, _admit_photons, _admit_stepped, _admit_tracked
from chroma_amd.tracks import host_tracks

# ---- refusals ----------------------------------------------------------------------------------------------------------
# Recorded on the commit before DaqChain (cb01f9e): the text of the ValueError for every set of given stages that violates one or
# two of the six dependencies, per caller.  A set is written by its stages' letters: w(indow) t(rigger) n(oise) (di)g(itizer)
# r(educer) s(eeder) d(irection).  acquire_pulses has the first four dependencies, and a missing window is a bad window to it.
LETTERS = dict(w='window', t='trigger', n='noise', g='digitizer', r='reducer', s='seeder', d='direction')
SIMULATE_REFUSES = {
    'daq_digitizer needs daq_trigger':
        'g gd gr grd grs grsd gs gsd wg wgd wgr wgrd wgrs wgrsd wgs wgsd wng wngd wngr wngrd wngrs wngrsd wngs wngsd',
    'daq_direction needs daq_seeder':
        'd wd wnd wtgd wtgrd wtd wtngd wtngrd wtnd',
    'daq_noise needs daq_window':
        'n ng ngr nd nr ns nsd',
    'daq_reducer needs daq_digitizer':
        'r rd rs rsd wnr wnrd wnrs wnrsd wr wrd wrs wrsd wtnr wtnrd wtnrs wtnrsd wtr wtrd wtrs wtrsd',
    'daq_seeder needs daq_trigger':
        's sd wns wnsd ws wsd',
    'daq_trigger needs daq_window':
        't tg tgd tgr tgrd tgrs tgrsd tgs tgsd td tn tng tngr tngrs tngrsd tngs tngsd tns tnsd tr trs trsd ts tsd',
}
ACQUIRE_REFUSES = {
    'a DAQ window is (t0, dt, nbins)':
        'g gr n ng ngr nr r t tg tgr tn tng tngr tr',
    'a digitiser reads the gates of a trigger: digitizer needs trigger':
        'wg wgr wng wngr',
    'a reducer reads the traces of a digitiser: reducer needs digitizer':
        'wnr wr wtnr wtr',
}
WINDOW = (-8.0, 0.5, 64)
VALUES = dict(window=WINDOW, trigger=(3, 4), noise=1000.0, digitizer=DaqDigitizer([1.0]), reducer=DaqReducer(5), seeder=200.0, direction=0.75)


def rows(table):
    return {word: message for message, words in table.items() for word in words.split()}


def violating(needs):
    """Every set of stages (as its word) that violates one or two of ``needs``."""
    letter = {stage: key for key, stage in LETTERS.items()}
    stages = ['window'] + [stage for stage, _ in needs]
    for r in range(len(stages) + 1):
        for given in itertools.combinations(stages, r):
            if 1 <= sum(1 for stage, need in needs if stage in given and need not in given) <= 2:
                yield ''.join(letter[stage] for stage in given)


def bare_simulation(**attributes):
    """(no context, no geometry: anything but the refusal fails on a missing attribute)"""
    sim = object.__new__(Simulation)
    sim.daq_seeder = sim.daq_direction = None
    for name, value in attributes.items():
        setattr(sim, name, value)
    return sim


def test_the_tables_hold_every_violation_of_one_or_two_dependencies():
    assert DAQ_NEEDS == (('trigger', 'window'), ('noise', 'window'), ('digitizer', 'trigger'), ('reducer', 'digitizer'), ('seeder', 'trigger'),
                         ('direction', 'seeder'))
    assert sorted(rows(SIMULATE_REFUSES)) == sorted(violating(DAQ_NEEDS)) and len(rows(SIMULATE_REFUSES)) == 90
    assert sorted(rows(ACQUIRE_REFUSES)) == sorted(violating(DAQ_NEEDS[:4])) and len(rows(ACQUIRE_REFUSES)) == 22


@pytest.mark.parametrize('word, message', sorted(rows(SIMULATE_REFUSES).items()))
def test_simulate_refuses_with_the_words_it_had(word, message):
    given = {'daq_' + LETTERS[key]: VALUES[LETTERS[key]] for key in word}
    with pytest.raises(ValueError) as e:
        next(bare_simulation().simulate([event.Photons()], run_daq=True, **given))
    assert str(e.value) == message


@pytest.mark.parametrize('word, message', sorted(rows(ACQUIRE_REFUSES).items()))
def test_acquire_pulses_refuses_with_the_words_it_had(word, message):
    given = {LETTERS[key]: VALUES[LETTERS[key]] for key in word if key != 'w'}
    with pytest.raises(ValueError) as e:
        object.__new__(GPUEventDaq).acquire_pulses(None, None, [0, 1], WINDOW if 'w' in word else None, **given)
    assert str(e.value) == message


def test_simulate_asks_for_run_daq_and_channels_after_the_needs_and_before_it_converts():
    # (recorded on the same commit, in this order)
    for kw, message in ((dict(daq_window=WINDOW), 'daq_window needs run_daq=True'),
                        (dict(daq_window=WINDOW, run_daq=True), 'daq_window needs a detector with channels'),
                        (dict(daq_window=WINDOW, daq_reducer=VALUES['reducer']), 'daq_reducer needs daq_digitizer'),
                        (dict(daq_window=(1, 2)), 'daq_window needs run_daq=True'),
                        (dict(daq_window=WINDOW, daq_trigger=(3, 4), daq_direction=0.75, run_daq=True), 'daq_direction needs daq_seeder')):
        with pytest.raises(ValueError) as e:
            next(bare_simulation(stepper=None).simulate([event.Photons()], **kw))
        assert str(e.value) == message


def test_the_constructor_s_direction_needs_its_seeder():
    with pytest.raises(ValueError) as e:
        Simulation(None, daq_direction=0.75)          # (refused before the detector or a GPU is looked at)
    assert str(e.value) == 'daq_direction needs daq_seeder'


class Once(DaqTrigger):
    """A trigger whose check passes once"""
    checks = 0

    def check(self, window):
        self.checks += 1
        if self.checks > 1:
            raise AssertionError('checked again')
        return DaqTrigger.check(self, window)


def test_a_resolved_chain_is_not_converted_or_checked_again():
    trigger = Once(3, 4)
    chain = DaqChain(WINDOW, trigger, 0.0, DaqDigitizer([1.0]), (5,))
    assert trigger.checks == 1 and chain.trigger is trigger and chain.noise is None and isinstance(chain.reducer, DaqReducer)
    assert chain.window == DaqChain(chain.window).window and chain.keep_traces is True
    daq = object.__new__(GPUEventDaq)
    # the chain goes through to the checks that depend on the call -- the bounds' is the first -- and the keywords are not looked at
    for _ in range(2):
        with pytest.raises(ValueError, match='bounds: a 1-D array'):
            daq.acquire_pulses(None, None, [[0, 1]], None, trigger='not a trigger', chain=chain)
    assert trigger.checks == 1
    # without one the keywords are resolved as before: the trigger is checked once more per call
    with pytest.raises(ValueError, match='bounds: a 1-D array'):
        daq.acquire_pulses(None, None, [[0, 1]], WINDOW, trigger=Once(3, 4))
    with pytest.raises(AssertionError, match='checked again'):
        daq.acquire_pulses(None, None, [[0, 1]], WINDOW, trigger=trigger)
    # what does not fit is refused where the chain is made, in the stages' order
    with pytest.raises(ValueError, match='a DAQ trigger of width 65 on a window of 64 bins'):
        DaqChain(WINDOW, (3, 65), digitizer=(1, 2))
    with pytest.raises(ValueError, match='3 dark rates for 5 channels'):
        DaqChain(WINDOW, noise=[1.0, 2.0, 3.0], nchannels=5)
    with pytest.raises(ValueError, match='reducer needs digitizer'):
        DaqChain(WINDOW, (3, 4), reducer=(5,))


# ---- the batch cutter --------------------------------------------------------------------------------------------------
class Fake(object):
    def __init__(self, weight):
        self.weight = weight


def admit_fake(ev, evid, index):
    ev.id, ev.index = evid, index
    return ev, ev.weight


def parents_loop(iterable, evid_start, photons_per_batch):
    """The loop simulate() had (its three copies differed in what ``nphotons`` counts)."""
    nphotons, batch, evid = 0, [], evid_start
    for ev in iterable:
        ev.id = evid
        evid += 1
        ev.index = len(batch)
        nphotons += ev.weight
        batch.append(ev)
        if nphotons >= photons_per_batch:
            yield batch
            nphotons, batch = 0, []
    if batch:
        yield batch


@pytest.mark.parametrize('weights', [[0, 5, 0, 10, 3, 3, 4, 25, 1], [], [25], [4, 6], [4, 6, 0, 0], [0, 0, 0], [9.5, 0.5, 3.0], [10, 10, 10]])
def test_cut_batches_cuts_as_the_loop_it_replaced(weights):
    def described(batches):
        return [[(ev.weight, ev.id, ev.index) for ev in batch] for batch in batches]
    got = described(cut_batches([Fake(w) for w in weights], 7, 10, admit_fake))
    assert got == described(parents_loop([Fake(w) for w in weights], 7, 10))
    assert [key[1] for batch in got for key in batch] == list(range(7, 7 + len(weights)))
    if weights == [0, 5, 0, 10, 3, 3, 4, 25, 1]:
        assert [[key[0] for key in batch] for batch in got] == [[0, 5, 0, 10], [3, 3, 4], [25], [1]]


def test_cut_batches_reads_no_further_than_the_batch_asked_for():
    taken = []

    def source():
        for w in [6, 6, 1, 20, 2]:
            taken.append(w)
            yield Fake(w)
    batches = cut_batches(source(), 0, 10, admit_fake)
    assert taken == []
    assert len(next(batches)) == 2 and taken == [6, 6]
    assert len(next(batches)) == 2 and taken == [6, 6, 1, 20]
    assert len(next(batches)) == 1 and next(batches, None) is None


def steps_of(n):
    z = np.zeros(n)
    return event.Steps(np.arange(n, dtype=float), z, z, z, np.ones(n), z, z, np.full(n, 100.0), z, z)


def test_the_three_paths_write_what_they_wrote_and_refuse_mixed_input_in_their_words():
    photons = lambda n: event.Photons(np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3)), np.full(n, 400.0))
    vertex = lambda steps=None: event.Vertex('mu-', (0, 0, 0), (1, 0, 0), 100.0, steps=steps, pdgcode=13)
    with_photons, with_steps, with_neither = (lambda: event.Event(photons_beg=photons(3)), lambda: event.Event(vertices=[vertex(steps_of(4))]),
                                              lambda: event.Event(vertices=[vertex()]))
    # photons: id, nphotons and the index in the batch as evidx; an event without photons has no length (after its id was written)
    batches = list(cut_batches([event.Event(photons_beg=photons(n)) for n in (3, 2, 4)], 5, 5, _admit_photons))
    assert [[(ev.id, ev.nphotons, ev.photons_beg.evidx.tolist()) for ev in batch] for batch in batches] == [[(5, 3, [0, 0, 0]), (6, 2, [1, 1])], [(7, 4, [0, 0, 0, 0])]]
    stray = with_steps()
    with pytest.raises(TypeError, match='NoneType'):
        list(cut_batches([with_photons(), stray], 5, 100, _admit_photons))
    assert stray.id == 6
    # steps: id and the segments with the index in the batch, weighed by the callback's count; refused before the id is written
    weigh = lambda segments: 2.0 * len(segments)
    batches = list(cut_batches([with_steps() for _ in range(3)], 5, 12, _admit_stepped(weigh)))
    assert [[(ev.id, len(seg), sorted(set(np.asarray(seg.evidx).tolist()))) for ev, seg in batch] for batch in batches] == [[(5, 3, [0]), (6, 3, [1])], [(7, 3, [0])]]
    for stray in (with_photons(), with_neither()):
        with pytest.raises(NotImplementedError) as e:
            list(cut_batches([with_steps(), stray], 5, 100, _admit_stepped(weigh)))
        assert str(e.value) == 'events with steps and events with photons (or with neither) in one simulate() call' and stray.id == 0

    # neither: the id, weighed by the stepper's bound
    class Bound(object):
        def expected_photons_at_most(self, vertices, media):
            return 7.0 * len(vertices)
    batches = list(cut_batches([with_neither() for _ in range(3)], 5, 14, _admit_tracked(Bound(), None)))
    assert [[ev.id for ev in batch] for batch in batches] == [[5, 6], [7]] and all(ev.nphotons is None for batch in batches for ev in batch)
    for stray in (with_photons(), with_steps()):
        with pytest.raises(NotImplementedError) as e:
            list(cut_batches([with_neither(), stray], 5, 100, _admit_tracked(Bound(), None)))
        assert str(e.value) == 'events to be tracked and events with photons or steps in one simulate() call' and stray.id == 0


# ---- the pure pieces ---------------------------------------------------------------------------------------------------
def hits_of(channels):
    n = len(channels)
    return event.Photons(np.arange(3 * n).reshape(n, 3), np.zeros((n, 3)), np.zeros((n, 3)), np.full(n, 400.0), t=np.arange(n), channel=channels)


@pytest.mark.parametrize('channels', [[], [4], [4, 4, 4], [0, 0, 3, 7, 7, 7], [2, 5, 5, 9], [1, 1, 2, 3, 3], [0, 1, 2]])
def test_hits_by_channel_slices_as_the_lines_it_was(channels):
    ev_hits = hits_of(channels)
    # (the parent's lines)
    ch = ev_hits.channel
    first = np.flatnonzero(np.concatenate(([True], ch[1:] != ch[:-1]))) if len(ch) else np.zeros(0, np.intp)
    last = np.append(first[1:], len(ch))
    want = {c: ev_hits[a:b] for c, a, b in zip(ch[first].tolist(), first.tolist(), last.tolist())}
    got = hits_by_channel(ev_hits)
    assert list(got) == list(want) == sorted(set(channels))
    for c in want:
        assert np.array_equal(got[c].t, want[c].t) and np.array_equal(got[c].pos, want[c].pos) and (got[c].channel == c).all()
        assert got[c].t.tolist() == [k for k, have in enumerate(channels) if have == c]


def parents_tracks(tracking, lo, hi):
    """The lines _simulate_batch had (chroma/sim.py:102-114)."""
    step_ids_list, step_photons_list = tracking
    tracks = [[] for _ in range(hi - lo)]
    for step_ids, step_photons in zip(step_ids_list, step_photons_list):
        mask = np.logical_and(step_ids >= lo, step_ids < hi)
        if np.count_nonzero(mask) == 0:
            break
        ids = step_ids[mask] - lo
        photons = step_photons[mask]
        for k, pid in enumerate(ids):
            tracks[pid].append(photons[k])
    return [event.Photons.join(t, concatenate=False) if len(t) > 0 else event.Photons() for t in tracks]


def test_host_tracks_assembles_as_the_lines_it_was_break_included():
    # two events in one batch, photons 0..2 and 3..6; photons die at different steps; event 0 is absent from step 2 and back in
    # step 3, which the loop never reaches for it: it ends at the first step without a photon of the event
    step_ids = [np.arange(7), np.array([0, 1, 2, 3, 4, 5, 6]), np.array([3, 5, 6]), np.array([1, 5]), np.array([5])]
    step_photons = []
    for k, ids in enumerate(step_ids):
        n = len(ids)
        step_photons.append(event.Photons(np.column_stack([ids, np.full(n, k), np.zeros(n)]), np.zeros((n, 3)), np.zeros((n, 3)), np.full(n, 400.0),
                                          t=10.0 * k + ids, flags=np.full(n, k)))
    bounds = np.array([0, 3, 7])
    lengths = []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        got, want = host_tracks(step_ids, step_photons, lo, hi), parents_tracks((step_ids, step_photons), lo, hi)
        assert len(got) == len(want) == hi - lo
        for a, b in zip(got, want):
            assert all(np.array_equal(getattr(a, name), getattr(b, name)) for name in ('pos', 't', 'flags', 'wavelengths', 'last_hit_triangles'))
        lengths.append([len(t) for t in got])
    assert lengths == [[2, 2, 2], [3, 2, 5, 3]]          # (photon 1 has 2 rows, not 3: the break)
    # no photons, no steps
    assert host_tracks([], [], 0, 0) == [] and [len(t) for t in host_tracks([], [], 0, 2)] == [0, 0]
