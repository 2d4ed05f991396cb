"""The vertex seed without a GPU: chroma_vertex_seed_host and VertexSeeder.fit_many against a restatement of the header's text
("vertex seed", include/chroma_hip.h) in Python integers -- math.isqrt, lists, no NumPy arithmetic -- bit for bit, every output
and the optional scores, each array guarded by sentinels behind its end.  ``seed_cases()`` is shared with tests/test_gpu_seed.py,
as the DAQ tests share theirs; ``expected(case)`` restates a case once per process.

Differences between a channel and a position.  The coordinate ranges of the contract (channels and candidates within 2^23, the
lattice within 2^23 (1 - 2^-8) of its candidate) admit a difference of 2^24 along an axis at level 0 and of less than 3 * 2^23 =
25 165 824 with the lattice, so (y^2, y, y) exists for y <= 4095 at level 0 and y <= 5016 in all: the cases take y in {1, 2, 1000,
4095} at level 0 and y = 4579 and k = 2^24 + 2^22 through a level-1 lattice point; y = 5791 and 5792 (y^2 of 2^25) cannot be
stated through the calls: tests/test_seed_arith.py holds the floor square root to its definition there, on the host.  Each of these fits has ONE bin of ONE tick, so a distance that is off by one loses its hit.

Recovery (test_recovery_...): 150 channels on a sphere of 1000 mm, light from (123.4, -210.7, 88.8) mm at 37.3 ns, 200 mm/ns,
default seeder (bins of 1 ns = 200 mm of flight, candidates 125 mm apart).  The restatement puts the seed at (125.25, -250.25, 125)
mm, 53.65 mm from the truth: the candidate next to it already has every hit under the shape's peak, and a tie stays
at the centre.  The test holds the code to the restatement's bits and the distance to twice that."""
import ctypes
import math
import random

import numpy as np
import pytest

from chroma_amd import _lib
from chroma_amd.seed import VertexSeeder

SENTINEL = 0xA5A5A5A5
GUARD = 8
OUTPUTS = ('best_pos', 'best_score', 'best_bin', 'best_cand', 'outside', 'level_score', 'scores')
CHROMA_ERR_INVALID = -1


# ---- the restatement (from the header's text) ----
def restate(case):
    p = case['seeder']
    slowness, bin_ticks, nbins, shape, step, L = p['slowness'], p['bin_ticks'], p['nbins'], list(p['shape'][:p['nshape']]), p['step'], p['nlevels']
    K = len(shape)
    pos, cand, offsets = case['channel_pos'], case['cand'], case['offsets']
    nchannels = len(pos)
    out = {name: [] for name in OUTPUTS}
    for f in range(len(offsets) - 1):
        rows = range(offsets[f], offsets[f + 1])
        hits = [(case['hit_channel'][i], case['hit_time'][i], case['hit_weight'][i]) for i in rows]
        tau0 = case['tau0'][f]

        def at(x):
            H = [0] * (nbins + K)
            outside = 0
            for c, t, w in hits:
                if not 0 <= c < nchannels:
                    outside += 1
                    continue
                d = math.isqrt(sum((a - b) ** 2 for a, b in zip(pos[c], x)))
                tau = t - ((d * slowness + 32768) >> 16)
                if tau < tau0 or (tau - tau0) // bin_ticks >= nbins:
                    outside += 1
                    continue
                H[(tau - tau0) // bin_ticks] += min(w, 255)
            A = [sum(shape[j] * H[s + j] for j in range(K)) for s in range(nbins)]
            score = max(A)
            return score, A.index(score), outside

        scores = [at(c)[0] for c in cand]
        best_cand = scores.index(max(scores))
        best = tuple(cand[best_cand])
        levels = [scores[best_cand]]
        for l in range(1, L + 1):
            s = step >> (l - 1)
            points = [(best[0] + (i - 2) * s, best[1] + (j - 2) * s, best[2] + (k - 2) * s) for k in range(5) for j in range(5) for i in range(5)]
            got = [at(x)[0] for x in points]
            top = max(got)
            m = 62 if got[62] == top else got.index(top)
            best = points[m]
            levels.append(top)
        score, bin, outside = at(best)
        for name, v in zip(OUTPUTS, (list(best), score, bin, best_cand, outside, levels, scores)):
            out[name].append(v)
    return out


_expected = {}


def expected(case):
    if case['name'] not in _expected:
        _expected[case['name']] = restate(case)
    return _expected[case['name']]


# ---- the cases ----
def seeder_of(slowness=65536, bin_ticks=1, nbins=16, shape=(1,), step=0, nlevels=0, nshape=None):
    shape = list(shape)
    return dict(slowness=slowness, bin_ticks=bin_ticks, nbins=nbins, nshape=len(shape) if nshape is None else nshape, step=step, nlevels=nlevels,
                shape=shape + [0] * (16 - len(shape)))


def case_of(name, seeder, channel_pos, cand, fits):
    """``fits``: a (tau0, [(channel, time, weight), ...]) per fit"""
    offsets, tau0, rows = [0], [], []
    for t0, hits in fits:
        tau0.append(t0)
        rows.extend(hits)
        offsets.append(len(rows))
    return dict(name=name, seeder=seeder, channel_pos=[tuple(c) for c in channel_pos], cand=[tuple(c) for c in cand], offsets=offsets, tau0=tau0,
                hit_channel=[r[0] for r in rows], hit_time=[r[1] for r in rows], hit_weight=[r[2] for r in rows])


def exact_tof(d, slowness):
    return (d * slowness + 32768) >> 16


def arithmetic_cases():
    cases = []
    # a bin of one tick: fit f is the one hit of channel f, timed for candidate f
    diffs = [(0, 0, 0)] + [(k, 0, 0) for k in (1, 2, 1000, 5791, 5792, 2 ** 24)] + [(y * y, y, y) for y in (1, 2, 1000, 4095)]
    cand = [(-2 ** 23, -y, -z) for _, y, z in diffs]
    pos = [(c[0] + d[0], c[1] + d[1], c[2] + d[2]) for c, d in zip(cand, diffs)]
    fits = [(-7, [(f, math.isqrt(sum(x * x for x in d)) - 7, 1)]) for f, d in enumerate(diffs)]
    cases.append(case_of('distances', seeder_of(nbins=1), pos, cand, fits))
    # the same through a lattice point of level 1: m = 62 - 2 (i = 0): two steps of 2^21 down the x axis
    for name, d in (('far_k', (2 ** 24 + 2 ** 22, 0, 0)), ('far_y', (4579 * 4579, 4579, 4579))):
        c = (-2 ** 23, 0, 0)
        p = (c[0] - 2 ** 22 + d[0], d[1], d[2])
        cases.append(case_of(name, seeder_of(nbins=1, step=2 ** 21, nlevels=1), [p], [c], [(3, [(0, math.isqrt(sum(x * x for x in d)) + 3, 1)])]))
    # the residual's edges: tau0, one before, the last tick of the last bin, one behind; a channel at the candidate (d = 0)
    cases.append(case_of('tau_edges', seeder_of(bin_ticks=4, nbins=8, shape=[1] * 8), [(5, 6, 7)], [(5, 6, 7)],
                         [(-100, [(0, -100, 1), (0, -101, 2), (0, -100 + 31, 4), (0, -100 + 32, 8)])]))
    # slowness 1: 32768 units are the rounding tie (one tick), 32767 none; and a product d * slowness = 32768 mod 65536 elsewhere
    cases.append(case_of('slowness_1', seeder_of(slowness=1, nbins=3, shape=[1, 1, 1]), [(32768, 0, 0), (32767, 0, 0), (98304, 0, 0)], [(0, 0, 0)],
                         [(0, [(0, 1, 1), (1, 1, 2), (2, 1, 4), (2, 2, 8)])]))
    cases.append(case_of('slowness_tie', seeder_of(slowness=3 * 32768, nbins=4, shape=[1, 2]), [(1, 0, 0), (3, 0, 0), (5, 0, 0)], [(0, 0, 0)],
                         [(0, [(0, 2, 1), (1, 5, 1), (2, 9, 1)])]))
    # slowness 2^24: 256 ticks a unit, a flight of 2^31 ticks from 2^23 units and of 2^32 from 2^24
    cases.append(case_of('slowness_max', seeder_of(slowness=2 ** 24, nbins=2, shape=[1, 1]), [(2 ** 23, 0, 0), (-2 ** 23, 0, 0)], [(0, 0, 0), (2 ** 23, 0, 0)],
                         [(-2 ** 31, [(0, 0, 1), (1, 1, 2), (1, 2 ** 31 - 1, 4), (0, -2 ** 31, 8)])]))
    return cases


def score_cases():
    one = [(0, 0, 0)]
    cases = [case_of('k1', seeder_of(nbins=10, shape=[7]), one, one, [(0, [(0, 3, 2), (0, 3, 3), (0, 9, 4)])]),
             case_of('k16', seeder_of(nbins=40, shape=list(range(1, 17))), one, one, [(0, [(0, b, b % 5 + 1) for b in range(0, 40, 3)])]),
             case_of('max_last', seeder_of(nbins=8, shape=[1, 2, 9]), one, one, [(0, [(0, 0, 1), (0, 1, 1), (0, 5, 1)])]),
             case_of('nbins_1', seeder_of(nbins=1, shape=[3, 200]), one, one, [(0, [(0, 0, 5), (0, 1, 5)])]),
             case_of('nbins_1024', seeder_of(nbins=1024, shape=[2] + [0] * 14 + [3]), one, one, [(0, [(0, 1023, 10), (0, 1008, 1), (0, 1024, 100)])]),
             case_of('weights', seeder_of(nbins=4, shape=[1]), one, one, [(0, [(0, 0, 0), (0, 1, 255), (0, 2, 256), (0, 3, 2 ** 32 - 1)])]),
             case_of('full', seeder_of(nbins=2, shape=[255]), one, one, [(0, [(0, 1, 255)] * 65535)]),
             case_of('no_channel', seeder_of(nbins=2, shape=[1]), one + [(1, 1, 1)], one, [(0, [(-1, 0, 9), (2, 0, 9), (1, 1, 3), (-2 ** 31, 0, 1), (2 ** 31 - 1, 0, 1)])])]
    assert expected(cases[6])['best_score'] == [255 * 65535 * 255]
    return cases


def search_cases():
    ring = [(300, 0, 0), (0, 300, 0), (0, 0, 300), (-300, 0, 0)]
    wide = seeder_of(bin_ticks=1000, nbins=4, shape=[1], step=8, nlevels=3)
    return [case_of('no_hits', seeder_of(step=64, nlevels=4), ring, [(7, 8, 9), (1, 2, 3)], [(0, []), (5, [])]),
            case_of('mirror', seeder_of(nbins=4), [(0, 0, 0)], [(100, 0, 0), (-100, 0, 0), (0, 50, 0)], [(0, [(0, 100, 3)])]),
            case_of('tie_centre', wide, ring, [(10, 10, 10)], [(-500, [(c, 0, 1) for c in range(4)])]),
            case_of('step_0', seeder_of(nbins=64, bin_ticks=4, step=0, nlevels=3, shape=[1, 2, 1]), ring, [(20, 0, 0), (0, 20, 0)], [(-10, [(c, 290 + c, 1) for c in range(4)])]),
            case_of('step_1', seeder_of(nbins=64, bin_ticks=2, step=1, nlevels=8, shape=[1, 2, 1]), ring, [(20, 0, 0), (0, 20, 0)], [(-10, [(c, 290 + 3 * c, 1) for c in range(4)])]),
            case_of('no_levels', seeder_of(nbins=64, bin_ticks=2, step=16, nlevels=0, shape=[1, 2, 1]), ring, [(20, 0, 0), (0, 20, 0)], [(-10, [(c, 290 + 3 * c, 1) for c in range(4)])])]


def random_case(name, rng, nfits, ncand, hit_counts, nlevels, nchannels=40):
    pos = [tuple(rng.randint(-4000, 4000) for _ in range(3)) for _ in range(nchannels)]
    cand = [tuple(rng.randint(-3000, 3000) for _ in range(3)) for _ in range(ncand)]
    K = rng.randint(1, 16)
    shape = [rng.randint(0, 255) for _ in range(K)]
    shape[rng.randrange(K)] = rng.randint(1, 255)
    p = seeder_of(slowness=rng.randint(20000, 90000), bin_ticks=rng.randint(1, 40), nbins=rng.randint(100, 400), shape=shape, step=rng.randint(0, 700), nlevels=nlevels)
    fits = []
    for f in range(nfits):
        n = hit_counts[f % len(hit_counts)]
        vertex, T = [rng.randint(-2500, 2500) for _ in range(3)], rng.randint(-10 ** 6, 10 ** 6)
        hits = []
        for _ in range(n):
            c = rng.randint(-1, nchannels)          # (both ends have no channel)
            d = math.isqrt(sum((a - b) ** 2 for a, b in zip(pos[c], vertex))) if 0 <= c < nchannels else 0
            hits.append((c, T + exact_tof(d, p['slowness']) + rng.choice([0, 0, 0, rng.randint(-30, 300), rng.randint(-10 ** 5, 10 ** 5)]), rng.randint(0, 300)))
        fits.append((T - rng.randint(0, 2000), hits))
    return case_of(name, p, pos, cand, fits)


def random_cases():
    rng = random.Random(20261021)
    return [random_case('random_1x1_5000', rng, 1, 1, [5000], 1),
            random_case('random_2x64', rng, 2, 64, [1025, 64], 1),
            random_case('random_2x257', rng, 2, 257, [65, 63], 2),
            random_case('random_1x63_1025', rng, 1, 63, [1025], 0),
            random_case('random_65x65', rng, 65, 65, [0, 1, 63, 64, 65], 2)]


def noise_free_case():
    """hit_time = T + tof to candidate 5 by the definition's arithmetic: that candidate, every weight under the shape's maximum"""
    rng = random.Random(7)
    pos = [tuple(rng.randint(-4000, 4000) for _ in range(3)) for _ in range(30)]
    cand = [tuple(rng.randint(-3000, 3000) for _ in range(3)) for _ in range(12)]
    p = seeder_of(slowness=65536, bin_ticks=1, nbins=64, shape=[1, 4, 9, 4, 1])
    T = 1234
    hits = [(c, T + exact_tof(math.isqrt(sum((a - b) ** 2 for a, b in zip(pos[c], cand[5]))), p['slowness']), c % 7 + 1) for c in range(30)]
    return case_of('noise_free', p, pos, cand, [(T - 20, hits)])


def seed_cases():
    return arithmetic_cases() + score_cases() + search_cases() + random_cases() + [noise_free_case()]


# ---- the calls ----
def struct_of(p):
    s = _lib.VertexSeeder(p['slowness'], p['bin_ticks'], p['nbins'], p['nshape'], p['step'], p['nlevels'])
    for j in range(16):
        s.shape[j] = p['shape'][j]
    return s


def case_arrays(case):
    """the case as the calls' input arrays, in argument order behind the seeder: (nchannels, channel_pos, ncand, cand, nfits, offsets,
    tau0, hit_channel, hit_time, hit_weight)"""
    a = lambda v, kind: np.ascontiguousarray(np.array(v, dtype=np.int64).astype(kind).reshape(-1))
    return (len(case['channel_pos']), a(case['channel_pos'], np.int32), len(case['cand']), a(case['cand'], np.int32), len(case['offsets']) - 1,
            a(case['offsets'], np.uint32), a(case['tau0'], np.int32), a(case['hit_channel'], np.int32), a(case['hit_time'], np.int32),
            a(case['hit_weight'], np.uint32))


def output_sizes(case, scores=True):
    n, L, ncand = len(case['offsets']) - 1, case['seeder']['nlevels'], len(case['cand'])
    return [3 * n, n, n, n, n, n * (L + 1), n * ncand if scores else None]


def guarded(sizes):
    return [None if n is None else np.full(n + GUARD, SENTINEL, dtype=np.uint32) for n in sizes]


def check_outputs(case, arrays, sizes, what):
    want = expected(case)
    for name, a, n in zip(OUTPUTS, arrays, sizes):
        if a is None:
            continue
        assert np.all(a[n:] == SENTINEL), (what, case['name'], name, 'wrote behind its end')
        flat = np.array(want[name], dtype=np.int64).reshape(-1)
        got = a[:n].view(np.int32).astype(np.int64) if name == 'best_pos' else a[:n].astype(np.int64)
        assert np.array_equal(got, flat), (what, case['name'], name, got[:12], flat[:12])


def call_host(case, scores=True, out=None):
    lib = _lib.load()
    ins = case_arrays(case)
    sizes = output_sizes(case, scores)
    out = guarded(sizes) if out is None else out
    s = struct_of(case['seeder'])
    rc = lib.chroma_vertex_seed_host(ctypes.byref(s), *([x if isinstance(x, int) else _lib.ptr(x) for x in ins] + [_lib.ptr(a) for a in out]))
    return rc, out, sizes


CASES = seed_cases()


@pytest.mark.parametrize('case', CASES, ids=[c['name'] for c in CASES])
def test_host_twin_is_the_restatement(case):
    rc, out, sizes = call_host(case)
    assert rc == 0, _lib.load().chroma_last_error()
    check_outputs(case, out, sizes, 'host')


def test_host_twin_without_scores():
    case = CASES[-1]
    rc, out, sizes = call_host(case, scores=False)
    assert rc == 0
    check_outputs(case, out, sizes, 'host')


def test_the_edges_show_what_they_are_for():
    """the restatement itself lands where the cases were aimed"""
    by = {c['name']: expected(c) for c in CASES if not c['name'].startswith('random')}
    assert by['distances']['best_score'] == [1] * 11 and by['distances']['outside'] == [0] * 11
    assert [s[f] for f, s in enumerate(by['distances']['scores'])] == [1] * 11
    for name in ('far_k', 'far_y'):
        assert by[name]['level_score'] == [[0, 1]] and by[name]['outside'] == [0] and by[name]['best_pos'][0][0] == -2 ** 23 - 2 ** 22
    assert by['tau_edges']['best_score'] == [5] and by['tau_edges']['outside'] == [2]
    assert by['slowness_1']['best_score'] == [1 + 2 + 8] and by['slowness_1']['outside'] == [1]          # (98304 + 32768 >> 16 = 2: time 1 is before tau0)
    assert by['slowness_max']['scores'] == [[1 + 2, 8]] and by['slowness_max']['outside'] == [3]
    assert by['nbins_1024']['best_score'] == [2 * 1 + 3 * 10] and by['nbins_1024']['best_bin'] == [1008] and by['nbins_1024']['outside'] == [1]
    assert by['max_last']['best_bin'] == [3] and by['max_last']['best_score'] == [9]
    assert by['weights']['best_score'] == [255] and by['weights']['best_bin'] == [1]
    assert by['no_channel']['outside'] == [4] and by['no_channel']['best_score'] == [3]
    assert by['no_hits']['best_cand'] == [0, 0] and by['no_hits']['best_pos'] == [[7, 8, 9]] * 2 and by['no_hits']['level_score'] == [[0] * 5] * 2
    assert by['mirror']['best_cand'] == [0] and by['mirror']['scores'][0][:2] == [3, 3]
    assert by['tie_centre']['best_pos'] == [[10, 10, 10]] and by['tie_centre']['level_score'] == [[4] * 4]
    assert by['step_0']['best_pos'][0] == list(CASES_BY_NAME['step_0']['cand'][by['step_0']['best_cand'][0]])
    nf = by['noise_free']
    assert nf['best_cand'] == [5] and nf['outside'] == [0] and nf['best_score'] == [9 * sum(c % 7 + 1 for c in range(30))]


CASES_BY_NAME = {c['name']: c for c in CASES}


@pytest.mark.parametrize('case', CASES, ids=[c['name'] for c in CASES])
def test_properties_of_the_definition(case):
    rc, out, sizes = call_host(case)
    assert rc == 0
    n, L, ncand = len(case['offsets']) - 1, case['seeder']['nlevels'], len(case['cand'])
    levels = out[5][:sizes[5]].reshape(n, L + 1).astype(np.int64)
    scores = out[6][:sizes[6]].reshape(n, ncand)
    assert np.all(np.diff(levels, axis=1) >= 0)
    assert np.array_equal(levels[:, 0], scores.max(axis=1))
    assert np.array_equal(levels[:, L], out[1][:n])


# ---- refusals ----
def small_case():
    return case_of('small', seeder_of(nbins=8, step=4, nlevels=2), [(0, 0, 0), (9, 9, 9)], [(1, 2, 3), (4, 5, 6)], [(0, [(0, 3, 1), (1, 4, 1)]), (0, [(1, 2, 1)])])


def refusals():
    """(name, what to change in the arguments of a small valid call); shared with the GPU file.  A change is a function of the
    dict {'seeder': struct fields, 'args': the list of case_arrays, 'out': the output list} that edits it in place."""
    def field(name, value):
        return lambda d: d['seeder'].__setitem__(name, value)

    def arg(i, value):
        return lambda d: d['args'].__setitem__(i, value)

    def out(i):
        return lambda d: d['out'].__setitem__(i, None)

    def shape(values, nshape):
        def f(d):
            d['seeder']['shape'] = list(values) + [0] * (16 - len(values))
            d['seeder']['nshape'] = nshape
        return f

    def coordinate(i, at, value):
        def f(d):
            d['args'][i] = d['args'][i].copy()
            d['args'][i][at] = value
        return f

    u32 = lambda v: np.array(v, dtype=np.uint32)
    r = [('slowness_0', field('slowness', 0)), ('slowness_big', field('slowness', 2 ** 24 + 1)), ('bin_ticks_0', field('bin_ticks', 0)),
         ('bin_ticks_big', field('bin_ticks', 2 ** 20 + 1)), ('nbins_0', field('nbins', 0)), ('nbins_big', field('nbins', 1025)),
         ('nshape_0', field('nshape', 0)), ('nshape_big', field('nshape', 17)), ('step_big', field('step', 2 ** 21 + 1)), ('nlevels_big', field('nlevels', 9)),
         ('shape_entry', shape([1, 256], 2)), ('shape_zero', shape([0, 0, 5], 2)),
         ('ncand_0', arg(2, 0)), ('ncand_big', arg(2, 2 ** 20 + 1)),
         ('nchannels_big', arg(0, (2 ** 32 - 1) // 3 + 1)),
         ('channel_coordinate', coordinate(1, 4, 2 ** 23 + 1)), ('channel_coordinate_low', coordinate(1, 0, -2 ** 23 - 1)),
         ('cand_coordinate', coordinate(3, 5, 2 ** 23 + 1)), ('cand_coordinate_low', coordinate(3, 0, -2 ** 31)),
         ('offsets_start', arg(5, u32([1, 2, 3]))), ('offsets_descend', arg(5, u32([0, 3, 2]))), ('offsets_long', arg(5, u32([0, 65536, 65536]))),
         ('null_cand', arg(3, None)), ('null_offsets', arg(5, None)), ('null_tau0', arg(6, None)), ('null_channel_pos', arg(1, None)),
         ('null_hit_channel', arg(7, None)), ('null_hit_time', arg(8, None)), ('null_hit_weight', arg(9, None))]
    r += [('null_' + name, out(i)) for i, name in enumerate(OUTPUTS[:6])]
    return r


def refused_call(change):
    case = small_case()
    d = dict(seeder=dict(case['seeder']), args=list(case_arrays(case)), out=guarded(output_sizes(case)))
    change(d)
    return case, d


@pytest.mark.parametrize('name,change', refusals(), ids=[r[0] for r in refusals()])
def test_host_refusals_write_nothing(name, change):
    lib = _lib.load()
    case, d = refused_call(change)
    s = struct_of(d['seeder'])
    rc = lib.chroma_vertex_seed_host(ctypes.byref(s), *([x if isinstance(x, int) else _lib.ptr(x) for x in d['args']] + [_lib.ptr(a) for a in d['out']]))
    assert rc == CHROMA_ERR_INVALID, name
    assert all(a is None or np.all(a == SENTINEL) for a in d['out']), name


def test_host_refuses_a_null_seeder_and_too_many_scores():
    lib = _lib.load()
    case = small_case()
    ins = [x if isinstance(x, int) else _lib.ptr(x) for x in case_arrays(case)]
    out = guarded(output_sizes(case))
    assert lib.chroma_vertex_seed_host(None, *(ins + [_lib.ptr(a) for a in out])) == CHROMA_ERR_INVALID
    # nfits * ncand = 2^32 with the scores asked for; fine without them (fits without hits)
    ncand, nfits = 2 ** 20, 2 ** 12
    cand, offsets, tau0 = np.zeros(3 * ncand, dtype=np.int32), np.zeros(nfits + 1, dtype=np.uint32), np.zeros(nfits, dtype=np.int32)
    big = [np.full(n, SENTINEL, dtype=np.uint32) for n in (3 * nfits, nfits, nfits, nfits, nfits, 3 * nfits, 8)]
    s = struct_of(case['seeder'])
    rc = lib.chroma_vertex_seed_host(ctypes.byref(s), 0, None, ncand, _lib.ptr(cand), nfits, _lib.ptr(offsets), _lib.ptr(tau0), None, None, None,
                                     *[_lib.ptr(a) for a in big])
    assert rc == CHROMA_ERR_INVALID and all(np.all(a == SENTINEL) for a in big)
    assert all(np.all(a == SENTINEL) for a in out)


def test_no_fits_is_ok_and_writes_nothing():
    lib = _lib.load()
    case = small_case()
    args = list(case_arrays(case))
    args[4] = 0
    out = guarded(output_sizes(case))
    s = struct_of(case['seeder'])
    rc = lib.chroma_vertex_seed_host(ctypes.byref(s), *([x if isinstance(x, int) else _lib.ptr(x) for x in args] + [_lib.ptr(a) for a in out]))
    assert rc == 0 and all(np.all(a == SENTINEL) for a in out)


# ---- the Python layer ----
def as_case(name, seeder, prepared):
    """a ``VertexSeeder`` and its ``prepare`` as a case for the restatement"""
    s = prepared.struct
    p = dict(slowness=s.slowness, bin_ticks=s.bin_ticks, nbins=s.nbins, nshape=s.nshape, step=s.step, nlevels=s.nlevels, shape=list(s.shape))
    return dict(name=name, seeder=p, channel_pos=[tuple(int(v) for v in c) for c in seeder.channel_pos], cand=[tuple(int(v) for v in c) for c in seeder.cand],
                offsets=[int(v) for v in prepared.offsets], tau0=[int(v) for v in prepared.tau0], hit_channel=[int(v) for v in prepared.channel],
                hit_time=[int(v) for v in prepared.time], hit_weight=[int(v) for v in prepared.weight])


def python_layer_fixture():
    rng = np.random.RandomState(11)
    positions = rng.uniform(-400.0, 400.0, size=(25, 3))
    seeder = VertexSeeder(positions, 190.0, bin_ns=0.8, spacing_mm=260.0, levels=3, ticks_per_bin=8, weights='npe')
    truth = rng.uniform(-200.0, 200.0, size=(3, 3))
    counts = [25, 0, 17]
    offsets = np.concatenate([[0], np.cumsum(counts)])
    channel, t, w = [], [], []
    for f, n in enumerate(counts):
        ch = rng.permutation(25)[:n]
        channel.extend(ch)
        t.extend(1000.0 * f - 3.7 + np.sqrt(((positions[ch] - truth[f]) ** 2).sum(axis=1)) / 190.0 + rng.normal(0.0, 0.5, size=n))
        w.extend(rng.uniform(0.0, 6.0, size=n))
    return seeder, offsets, np.array(channel), np.array(t), np.array(w)


def test_fit_many_is_the_restatement_and_its_units():
    seeder, offsets, channel, t, w = python_layer_fixture()
    fits = seeder.fit_many(offsets, channel, t, w, scores=True)
    prepared = seeder.prepare(offsets, channel, t, w)
    # the quantisation, restated: ticks by floor(t / tick + 0.5) from the fit's earliest tick, tau0 the crossing of the sphere
    tick = 0.8 / 8
    for f in range(3):
        rows = slice(offsets[f], offsets[f + 1])
        ticks = [math.floor(x / tick + 0.5) for x in t[rows]]
        assert [int(v) for v in prepared.time[rows]] == [x - min(ticks) for x in ticks]
        assert int(prepared.origin[f]) == (min(ticks) if ticks else 0)
    radius = float(np.sqrt(((seeder.channel_pos * 0.125 - (seeder.channel_pos * 0.125).mean(axis=0)) ** 2).sum(axis=1)).max())
    assert abs(seeder.radius - radius) < 0.2
    assert list(prepared.tau0) == [-((math.ceil(2.0 * seeder.radius / 0.125) * seeder.slowness + 32768) >> 16)] * 3
    assert [int(v) for v in prepared.weight] == [math.floor(x + 0.5) for x in w]
    assert seeder.slowness == math.floor(65536.0 * 0.125 / (190.0 * tick) + 0.5) and seeder.step == 1040
    want = expected(as_case('python_layer', seeder, prepared))
    assert fits.pos_int.tolist() == want['best_pos'] and fits.score.tolist() == want['best_score'] and fits.bin.tolist() == want['best_bin']
    assert fits.cand.tolist() == want['best_cand'] and fits.outside.tolist() == want['outside'] and fits.level_score.tolist() == want['level_score']
    assert fits.scores.tolist() == want['scores'] and fits.nhits.tolist() == [25, 0, 17]
    assert np.array_equal(fits.pos, fits.pos_int * 0.125)
    peak = int(np.argmax(seeder.shape))
    for f in range(3):
        assert fits.t0[f] == (int(prepared.origin[f]) + int(prepared.tau0[f]) + (want['best_bin'][f] + peak) * 8) * tick
    one = seeder.fit(channel[:25], t[:25], w[:25])
    assert one.pos_int.tolist() == want['best_pos'][:1] and one.score.tolist() == want['best_score'][:1]
    assert fits[2:3].pos_int.tolist() == want['best_pos'][2:]


def test_seeder_construction():
    assert VertexSeeder.gaussian_shape(1.0, 1.0) == [3, 35, 155, 255, 155, 35, 3]
    tail = VertexSeeder.gaussian_shape(0.5, 1.0, tail_ns=2.0)
    assert len(tail) <= 16 and max(tail) == 255 and tail.index(255) == 1 and tail[2] == math.floor(255.0 * math.exp(-0.5) + 0.5)

    class Detector(object):
        channel_index_to_position = [np.array([100.0, 0.0, 0.0]), None, np.array([-100.0, 0.0, 0.0]), np.array([0.0, 100.0, 0.0]), np.array([0.0, -100.0, 0.0])]

    s = VertexSeeder.for_detector(Detector(), 200.0)
    assert s.channel_pos.tolist() == [[800, 0, 0], [0, 0, 0], [-800, 0, 0], [0, 800, 0], [0, -800, 0]]
    assert s.radius == 100.0 and s.spacing == 12.5 and s.step == 50 and s.levels == 6
    inside = [(i, j, k) for i in range(-8, 9) for j in range(-8, 9) for k in range(-8, 9) if i * i + j * j + k * k <= 64]
    assert len(s.cand) == len(inside) and set(map(tuple, s.cand.tolist())) == {(100 * i, 100 * j, 100 * k) for i, j, k in inside}
    with pytest.raises(ValueError):
        VertexSeeder(np.array([[2.0 ** 21, 0.0, 0.0]]), 200.0)
    with pytest.raises(ValueError):
        VertexSeeder(np.zeros((1, 3)), 200.0, weights='charge')
    with pytest.raises(ValueError):
        s.fit_many([0, 2], [0, 1], [0.0, float('nan')])


# ---- recovery ----
RECORDED_MM = 53.65          # the restatement's distance between truth and seed (this file's docstring)


def recovery_fixture():
    n = 150
    k = np.arange(n) + 0.5
    polar, azimuth = np.arccos(1.0 - 2.0 * k / n), math.pi * (1.0 + 5.0 ** 0.5) * k
    positions = 1000.0 * np.stack([np.sin(polar) * np.cos(azimuth), np.sin(polar) * np.sin(azimuth), np.cos(polar)], axis=1)
    truth = np.array([123.4, -210.7, 88.8])
    t = 37.3 + np.sqrt(((positions - truth) ** 2).sum(axis=1)) / 200.0
    return VertexSeeder(positions, 200.0), truth, np.arange(n), t


def test_recovery_of_an_off_lattice_noise_free_vertex():
    seeder, truth, channel, t = recovery_fixture()
    prepared = seeder.prepare([0, len(t)], channel, t)
    want = expected(as_case('recovery', seeder, prepared))
    assert want['outside'] == [0]
    distance = math.sqrt(sum((0.125 * a - b) ** 2 for a, b in zip(want['best_pos'][0], truth)))
    print('recovery: restated seed %s, %.3f mm from the truth, score %d of %d' % (want['best_pos'][0], distance, want['best_score'][0], 255 * len(t)))
    fit = seeder.fit(channel, t)
    assert fit.pos_int.tolist() == want['best_pos'] and fit.score.tolist() == want['best_score'] and fit.bin.tolist() == want['best_bin']
    assert fit.level_score.tolist() == want['level_score'] and fit.outside.tolist() == [0]
    assert float(np.sqrt(((fit.pos[0] - truth) ** 2).sum())) <= 2.0 * RECORDED_MM
    assert abs(distance - RECORDED_MM) < 0.005          # (the record is the restatement's figure)
