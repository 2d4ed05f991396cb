"""The direction seed without a GPU: chroma_direction_seed_host and DirectionSeeder.fit_many against a restatement of the header's
text ("direction seed", include/chroma_hip.h) in Python integers -- math.isqrt, abs(a) // b with the sign put back, lists, no NumPy
arithmetic -- bit for bit, every output and cos_hist, each array between sentinel words in front and behind.  ``dir_cases()`` is shared
with tests/test_gpu_dirseed.py; ``expected(case)`` restates a case once per process.

The ring (test_the_ring_...): 2000 channels on a Fibonacci sphere of 1000 mm, seen from (123.4, -210.7, 88.8) mm; unit-weight hits
on every channel whose cosine to the axis (0.3, -0.5, 0.81) / |.| is within 0.05 of 0.75; cherenkov_profile(0.75, 0.05), grid 12,
6 levels.  The restatement's axis lies 1.39 degrees from the truth; the level-0 grid's covering angle -- the
farthest a direction can lie from its nearest candidate, taken at the corners of the grid's cells -- is 5.29 degrees (cells of 7.5 degrees: 7.5 / sqrt 2).  The test
holds the code to the restatement's bits and the angle to that covering angle, no tighter."""
import ctypes
import math
import random

import numpy as np
import pytest

from chroma_amd import _lib
from chroma_amd.seed import DirectionSeeder, DirFits, SeedFits, VertexSeeder, to_vertices

SENTINEL = 0xA5A5A5A5
GUARD = 8
OUTPUTS = ('best_dir', 'best_score', 'best_cand', 'inside', 'outside', 'level_score', 'cos_hist')
CHROMA_ERR_INVALID = -1
ONE = 16384


# ---- the restatement (from the header's text) ----
def trunc_div(a, b):
    """C's a / b for b > 0: toward zero"""
    q = abs(a) // b
    return -q if a < 0 else q


def unit_of(a):
    length = math.isqrt(sum(x * x for x in a))
    return (0, 0, 0) if length == 0 else tuple(trunc_div(x * ONE, length) for x in a)


def restate(case):
    p, t = case['seeder'], case['timing']
    m, step, L, first, width, profile = p['log2_ncos'], p['step'], p['nlevels'], p['first'], p['width'], p['profile']
    pos, cand, offsets = case['channel_pos'], case['cand'], case['offsets']
    timed = case['hit_time'] is not None
    out = {name: [] for name in OUTPUTS}
    for f in range(len(offsets) - 1):
        v = case['vertex'][f]
        records, inside, outside = [], 0, 0
        for i in range(offsets[f], offsets[f + 1]):
            c, w = case['hit_channel'][i], case['hit_weight'][i]
            if not 0 <= c < len(pos):
                outside += 1
                continue
            delta = [a - b for a, b in zip(pos[c], v)]
            d = math.isqrt(sum(x * x for x in delta))
            if d == 0:
                outside += 1
                continue
            if timed:
                r = case['hit_time'][i] - ((d * t['slowness'] + 32768) >> 16) - case['tau0'][f]
                if r < 0 or r >= t['nbins'] * t['bin_ticks']:
                    outside += 1
                    continue
                b = r // t['bin_ticks']
                if b < case['bin'][f] + first or b >= case['bin'][f] + first + width:
                    outside += 1
                    continue
            w = min(w, 255)
            inside += w
            records.append((w, tuple(trunc_div(x * ONE, d) for x in delta)))

        def k_of(n, u):
            c = max(-ONE, min(ONE - 1, (n[0] * u[0] + n[1] * u[1] + n[2] * u[2]) >> 14))
            return (c + ONE) >> (15 - m)

        def score(u):
            return 0 if u == (0, 0, 0) else sum(w * profile[k_of(n, u)] for w, n in records)

        units = [unit_of(a) for a in cand]
        scores = [score(u) for u in units]
        best_cand = scores.index(max(scores))
        best = units[best_cand]
        levels = [scores[best_cand]]
        for l in range(1, L + 1):
            s = step >> (l - 1)
            points = [unit_of((best[0] + (i - 2) * s, best[1] + (j - 2) * s, best[2] + (k - 2) * s)) for k in range(5) for j in range(5) for i in range(5)]
            points[62] = best          # (the centre as it is)
            got = [score(u) for u in points]
            top = max(got)
            best = points[62 if got[62] == top else got.index(top)]
            levels.append(top)
        hist = [0] * (1 << m)
        for w, n in records:
            hist[k_of(n, best)] += w
        for name, value in zip(OUTPUTS, (list(best), levels[-1], best_cand, inside, outside, levels, hist)):
            out[name].append(value)
    return out


_expected = {}


def expected(case):
    if case['name'] not in _expected:
        _expected[case['name']] = restate(case)
    return _expected[case['name']]


# ---- the cases ----
def peaked(m, k, value=255):
    return [value if j == k else 0 for j in range(1 << m)] + [0] * (256 - (1 << m))


def seeder_of(log2_ncos=6, step=0, nlevels=0, first=0, width=1, profile=None):
    profile = list(profile) if profile is not None else [(7 * k * k + 3) % 256 for k in range(1 << log2_ncos)]
    return dict(log2_ncos=log2_ncos, step=step, nlevels=nlevels, first=first, width=width, profile=profile + [0] * (256 - len(profile)))


def timing_of(slowness=65536, bin_ticks=1, nbins=16):
    return dict(slowness=slowness, bin_ticks=bin_ticks, nbins=nbins)


def case_of(name, seeder, channel_pos, cand, fits, timing=None):
    """``fits``: a (vertex, tau0, bin, [(channel, time, weight), ...]) per fit; with ``timing`` None the times are not passed"""
    offsets, tau0, vertex, bins, rows = [0], [], [], [], []
    for v, t0, b, hits in fits:
        vertex.append(tuple(v))
        tau0.append(t0)
        bins.append(b)
        rows.extend(hits)
        offsets.append(len(rows))
    return dict(name=name, seeder=seeder, timing=timing if timing is not None else timing_of(), channel_pos=[tuple(c) for c in channel_pos],
                cand=[tuple(c) for c in cand], offsets=offsets, tau0=tau0, vertex=vertex, bin=bins, hit_channel=[r[0] for r in rows],
                hit_time=[r[1] for r in rows] if timing is not None else None, hit_weight=[r[2] for r in rows])


AXES = [(ONE, 0, 0), (-ONE, 0, 0), (0, ONE, 0), (0, -ONE, 0), (0, 0, ONE), (0, 0, -ONE)]
CORNERS = [(x, y, z) for x in (-9000, 9000) for y in (-9000, 9000) for z in (-9000, 9000)]


def edge_cases():
    origin = (0, 0, 0)
    ring = [(300, 0, 400), (-300, 0, 400), (0, 300, 400), (0, -300, 400), (5, 6, 7)]
    top = 2 ** 23
    cases = []
    # the time cut: bins of 4 ticks from tau0 = -100, the window [bin + first, + width) = [3, 5): residuals 12 .. 19
    tm = timing_of(bin_ticks=4, nbins=8)
    hits = [(0, 500 - 100 + r, 1 << j) for j, r in enumerate((-1, 0, 11, 12, 19, 20, 31, 32))]
    cases.append(case_of('window', seeder_of(first=2, width=2, step=512, nlevels=2), ring, AXES, [(origin, -100, 1, hits)], tm))
    # a window that excludes every hit: behind the last bin, and a bin word whose sum with `first` passes 2^32
    cases.append(case_of('window_none', seeder_of(first=1040, width=2048, step=64, nlevels=2), ring, AXES,
                         [(origin, -100, 8, hits), (origin, -100, 2 ** 32 - 1, hits)], tm))
    # a channel at the vertex (d = 0), channels -1 and nchannels and the ends of int32
    cases.append(case_of('no_direction', seeder_of(step=100, nlevels=1), ring, AXES,
                         [((5, 6, 7), 0, 0, [(4, 0, 9), (0, 0, 2), (-1, 0, 9), (5, 0, 9), (-2 ** 31, 0, 1), (2 ** 31 - 1, 0, 1), (2, 0, 3)])]))
    cases.append(case_of('weights', seeder_of(log2_ncos=4, profile=[1] * 16), ring, AXES[:1], [(origin, 0, 0, [(0, 0, 0), (1, 0, 255), (2, 0, 256), (3, 0, 2 ** 32 - 1)])]))
    # coordinates at +-2^23, candidate components at +-2^15: a difference of 2^24 along every axis, with and without the flight
    far = [(top, -top, top), (-top, top, -top), (top, top, top), (-top, -top, top), (top, 0, 0)]
    big = [(2 ** 15, -2 ** 15, 2 ** 15), (-2 ** 15, 2 ** 15, -2 ** 15), (2 ** 15, 2 ** 15, 2 ** 15), (2 ** 15, 0, 0), (-2 ** 15, -2 ** 15, 2 ** 15)]
    cases.append(case_of('extremes', seeder_of(log2_ncos=8, step=2 ** 13, nlevels=2), far, big,
                         [((-top, top, -top), 0, 0, [(c, 0, c + 1) for c in range(5)]), ((top, -top, top), 0, 0, [(c, 0, 7) for c in range(5)])]))
    flight = lambda a, b: math.isqrt(sum((x - y) ** 2 for x, y in zip(a, b)))
    v = (-top, top, -top)
    cases.append(case_of('extremes_timed', seeder_of(log2_ncos=8, step=2 ** 13, nlevels=1, first=0, width=1), far, big,
                         [(v, -2 ** 31, 5, [(c, -2 ** 31 + 40 * flight(far[c], v) + 5 + (c == 3), 3) for c in range(5)])],
                         timing_of(slowness=40 * 65536, bin_ticks=1, nbins=1024)))
    # a (0, 0, 0) candidate alone -- it stays without a step and leaves with one -- and beside others
    cases.append(case_of('zero_alone', seeder_of(step=0, nlevels=3), ring, [origin], [(origin, 0, 0, [(c, 0, 1) for c in range(4)])]))
    cases.append(case_of('zero_alone_step', seeder_of(step=2 ** 13, nlevels=3, profile=peaked(6, 57)), ring, [origin], [(origin, 0, 0, [(c, 0, 1) for c in range(4)])]))
    cases.append(case_of('zero_beside', seeder_of(step=300, nlevels=2), ring, [origin, (0, 0, 1), origin, (3, 0, -4)], [(origin, 0, 0, [(c, 0, 2) for c in range(4)])]))
    # a constant profile: every point ties, the lowest candidate wins and the centre keeps every level
    cases.append(case_of('constant', seeder_of(log2_ncos=5, step=2 ** 13, nlevels=8, profile=[7] * 32), ring, CORNERS + [(1, 2, 3)],
                         [(origin, 0, 0, [(c, 0, c + 1) for c in range(5)])]))
    # mirror-symmetric hits about the candidate's axis under a profile of the top bin alone: the centre sees neither hit there, the
    # points towards either do, and the lowest m of the tied takes the level
    cases.append(case_of('mirror', seeder_of(log2_ncos=8, step=1500, nlevels=1, profile=peaked(8, 255)), [(300, 0, 1600), (-300, 0, 1600)], [(0, 0, 5)],
                         [(origin, 0, 0, [(0, 0, 3), (1, 0, 3)])]))
    # nlevels 8 at log2_ncos 4 with the greatest step, and step 0 under levels
    cases.append(case_of('levels_8', seeder_of(log2_ncos=4, step=2 ** 13, nlevels=8, profile=[0, 0, 0, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 255]), ring, AXES,
                         [((40, -30, -200), 0, 0, [(c, 0, 10 * c + 1) for c in range(5)])]))
    cases.append(case_of('step_0', seeder_of(step=0, nlevels=8), ring, AXES, [((40, -30, -200), 0, 0, [(c, 0, 10 * c + 1) for c in range(5)])]))
    cases.append(case_of('no_hits', seeder_of(step=64, nlevels=4), ring, AXES, [(origin, 0, 0, []), ((1, 2, 3), 5, 7, [])], tm))
    return cases


def random_case(name, rng, hit_counts, ncand, nlevels, log2_ncos, step, timed, nchannels=60):
    pos = [tuple(rng.randint(-4000, 4000) for _ in range(3)) for _ in range(nchannels)]
    cand = [tuple(rng.randint(-2 ** 15, 2 ** 15) for _ in range(3)) for _ in range(ncand)]
    profile = [rng.randint(0, 255) for _ in range(1 << log2_ncos)]
    profile[rng.randrange(1 << log2_ncos)] = rng.randint(1, 255)
    tm = timing_of(slowness=rng.randint(20000, 90000), bin_ticks=rng.randint(1, 40), nbins=rng.randint(100, 400))
    p = seeder_of(log2_ncos, step, nlevels, first=rng.randint(0, 4), width=rng.randint(1, 12), profile=profile)
    fits = []
    for n in hit_counts:
        vertex, T = [rng.randint(-2500, 2500) for _ in range(3)], rng.randint(-10 ** 6, 10 ** 6)
        b = rng.randint(0, 20)
        hits = []
        for _ in range(n):
            c = rng.randint(-1, nchannels)          # (both ends have no channel)
            d = math.isqrt(sum((a - x) ** 2 for a, x in zip(pos[c], vertex))) if 0 <= c < nchannels else 0
            late = rng.choice([0, 0, 0, rng.randint(-30, 300), rng.randint(-10 ** 5, 10 ** 5)])
            hits.append((c, T + ((d * tm['slowness'] + 32768) >> 16) + (b + p['first']) * tm['bin_ticks'] + late, rng.randint(0, 300)))
        fits.append((vertex, T, b, hits))
    return case_of(name, p, pos, cand, fits, tm if timed else None)


def random_cases():
    rng = random.Random(20261021)
    return [random_case('random_sizes', rng, [0, 1, 63, 64, 65, 511, 512, 513, 1025], 9, 1, 6, 700, True),
            random_case('random_sizes_untimed', rng, [513, 0, 1025, 64], 8, 1, 5, 2000, False),
            random_case('random_1cand_8levels', rng, [65], 1, 8, 4, 2 ** 13, False),
            random_case('random_7cand', rng, [64, 513], 7, 2, 8, 300, True),
            random_case('random_64cand', rng, [63, 512], 64, 0, 8, 300, False),
            random_case('random_65fits', rng, [0, 1, 63, 64, 65] * 13, 17, 1, 6, 1000, True)]


def dir_cases():
    return edge_cases() + random_cases()


# ---- the calls ----
def struct_of(p):
    s = _lib.DirectionSeeder(p['log2_ncos'], p['step'], p['nlevels'], p['first'], p['width'])
    for k in range(256):
        s.profile[k] = p['profile'][k]
    return s


def timing_struct(t):
    return _lib.VertexSeeder(t['slowness'], t['bin_ticks'], t['nbins'], 1, 0, 0)


def case_arrays(case):
    """the case as the calls' input arrays, in argument order behind the seeder and the timing: (nchannels, channel_pos, ncand, cand,
    nfits, offsets, tau0, vertex, bin, hit_channel, hit_time or None, hit_weight)"""
    a = lambda v, kind: np.ascontiguousarray(np.array(v, dtype=np.int64).astype(kind).reshape(-1))
    return (len(case['channel_pos']), a(case['channel_pos'], np.int32), len(case['cand']), a(case['cand'], np.int32), len(case['offsets']) - 1,
            a(case['offsets'], np.uint32), a(case['tau0'], np.int32), a(case['vertex'], np.int32), a(case['bin'], np.uint32), a(case['hit_channel'], np.int32),
            None if case['hit_time'] is None else a(case['hit_time'], np.int32), a(case['hit_weight'], np.uint32))


def output_sizes(case, cos_hist=True):
    n, L, m = len(case['offsets']) - 1, case['seeder']['nlevels'], case['seeder']['log2_ncos']
    return [3 * n, n, n, n, n, n * (L + 1), n << m if cos_hist else None]


def guarded(sizes):
    """an array per output with GUARD sentinel words in front of it and behind: the calls get the address of word GUARD"""
    return [None if n is None else np.full(n + 2 * GUARD, SENTINEL, dtype=np.uint32) for n in sizes]


def body(a, n):
    return a[GUARD:GUARD + n]


def check_outputs(case, arrays, sizes, what):
    want = expected(case)
    for name, a, n in zip(OUTPUTS, arrays, sizes):
        if a is None:
            continue
        assert np.all(a[:GUARD] == SENTINEL), (what, case['name'], name, 'wrote in front of its start')
        assert np.all(a[GUARD + n:] == SENTINEL), (what, case['name'], name, 'wrote behind its end')
        flat = np.array(want[name], dtype=np.int64).reshape(-1)
        got = body(a, n).view(np.int32).astype(np.int64) if name == 'best_dir' else body(a, n).astype(np.int64)
        assert np.array_equal(got, flat), (what, case['name'], name, got[:12], flat[:12])


def host_call(seeder, timing, args, out):
    lib = _lib.load()
    s = None if seeder is None else ctypes.byref(struct_of(seeder))
    t = None if timing is None else ctypes.byref(timing_struct(timing))
    return lib.chroma_direction_seed_host(s, t, *([x if isinstance(x, int) else _lib.ptr(x) for x in args] + [None if a is None else _lib.ptr(a[GUARD:]) for a in out]))


def call_host(case, cos_hist=True):
    sizes = output_sizes(case, cos_hist)
    out = guarded(sizes)
    return host_call(case['seeder'], case['timing'], case_arrays(case), out), out, sizes


CASES = dir_cases()
CASES_BY_NAME = {c['name']: c for c in CASES}


@pytest.mark.parametrize('case', CASES, ids=[c['name'] for c in CASES])
def test_host_twin_is_the_restatement(case):
    rc, out, sizes = call_host(case)
    assert rc == 0, _lib.load().chroma_last_error()
    check_outputs(case, out, sizes, 'host')


def test_host_twin_without_cos_hist():
    case = CASES_BY_NAME['random_7cand']
    rc, out, sizes = call_host(case, cos_hist=False)
    assert rc == 0
    check_outputs(case, out, sizes, 'host')


def test_the_table_covers_what_it_is_for():
    counts = {n for c in CASES for n in np.diff(c['offsets']).tolist()}
    assert {0, 1, 63, 64, 65, 511, 512, 513, 1025} <= counts
    assert {1, 7, 8, 9, 64} <= {len(c['cand']) for c in CASES}
    for key, values in (('nlevels', {0, 8}), ('log2_ncos', {4, 8}), ('step', {0, 2 ** 13})):
        assert values <= {c['seeder'][key] for c in CASES}, key
    assert {True, False} == {c['hit_time'] is None for c in CASES}


def test_the_edges_show_what_they_are_for():
    """the restatement itself lands where the cases were aimed"""
    by = {c['name']: expected(c) for c in CASES if not c['name'].startswith('random')}
    assert by['window']['inside'] == [8 + 16] and by['window']['outside'] == [6]
    assert by['window_none']['inside'] == [0, 0] and by['window_none']['outside'] == [8, 8] and by['window_none']['best_cand'] == [0, 0]
    assert by['window_none']['level_score'] == [[0] * 3] * 2 and by['window_none']['best_dir'] == [[ONE, 0, 0]] * 2
    assert by['no_direction']['outside'] == [5] and by['no_direction']['inside'] == [5]
    assert by['weights']['inside'] == [0 + 255 + 255 + 255] and by['weights']['best_score'] == [765] and by['weights']['outside'] == [0]
    assert by['extremes']['outside'] == [1, 1] and by['extremes']['inside'] == [1 + 3 + 4 + 5, 28]          # (the channel at the vertex)
    assert by['extremes_timed']['inside'] == [3 * 3] and by['extremes_timed']['outside'] == [2]          # (the vertex's own channel, the late one)
    assert by['zero_alone']['best_dir'] == [[0, 0, 0]] and by['zero_alone']['level_score'] == [[0] * 4] and by['zero_alone']['inside'] == [4]
    assert sum(by['zero_alone']['cos_hist'][0]) == 4 and by['zero_alone']['cos_hist'][0][32] == 4
    assert by['zero_alone_step']['best_dir'] != [[0, 0, 0]] and by['zero_alone_step']['level_score'][0][0] == 0 and by['zero_alone_step']['best_score'][0] > 0
    assert by['zero_beside']['best_cand'][0] in (1, 3) and by['zero_beside']['level_score'][0][0] > 0
    const = by['constant']
    assert const['best_cand'] == [0] and const['level_score'] == [[7 * 15] * 9] and const['best_dir'] == [list(unit_of(CORNERS[0]))]
    mirror = by['mirror']
    assert mirror['level_score'] == [[0, 3 * 255]] and mirror['best_dir'][0][0] < 0          # (its image under x -> -x, a higher m, scores the same bit for bit)
    assert by['step_0']['best_dir'] == [list(AXES[by['step_0']['best_cand'][0]])] and len(set(by['step_0']['level_score'][0])) == 1
    assert len(set(by['levels_8']['level_score'][0])) > 2
    assert by['no_hits']['best_cand'] == [0, 0] and by['no_hits']['best_dir'] == [[ONE, 0, 0]] * 2 and by['no_hits']['level_score'] == [[0] * 5] * 2


@pytest.mark.parametrize('case', CASES, ids=[c['name'] for c in CASES])
def test_properties_of_the_definition(case):
    rc, out, sizes = call_host(case)
    assert rc == 0
    n, L, m = len(case['offsets']) - 1, case['seeder']['nlevels'], case['seeder']['log2_ncos']
    levels = body(out[5], sizes[5]).reshape(n, L + 1).astype(np.int64)
    assert np.all(np.diff(levels, axis=1) >= 0)
    assert np.array_equal(levels[:, L], body(out[1], n))
    inside, outside, nhits = body(out[3], n).astype(np.int64), body(out[4], n).astype(np.int64), np.diff(case['offsets'])
    assert np.array_equal(body(out[6], sizes[6]).reshape(n, 1 << m).astype(np.int64).sum(axis=1), inside)
    assert np.all(inside <= 255 * (nhits - outside)) and np.all(outside <= nhits)
    assert np.all(np.abs(body(out[0], 3 * n).view(np.int32)) <= ONE)


# ---- refusals ----
def small_case():
    return case_of('small', seeder_of(step=40, nlevels=2, first=0, width=8), [(0, 0, 90), (9, 9, 9)], [(1, 2, 3), (4, 5, 6)],
                   [((1, 1, 1), 0, 0, [(0, 90, 1), (1, 14, 1)]), ((2, 2, 2), 0, 0, [(1, 12, 1)])], timing_of())


def refusals():
    """(name, what to change in the arguments of a small valid call with times); shared with the GPU file.  A change is a function of
    the dict {'seeder': struct fields or None, 'timing': likewise, 'args': the list of case_arrays, 'out': the output list} that
    edits it in place."""
    def field(name, value, of='seeder'):
        return lambda d: d[of].__setitem__(name, value)

    def arg(i, value):
        return lambda d: d['args'].__setitem__(i, value)

    def out(i):
        return lambda d: d['out'].__setitem__(i, None)

    def whole(of):
        return lambda d: d.__setitem__(of, None)

    def coordinate(i, at, value):
        def f(d):
            d['args'][i] = d['args'][i].copy()
            d['args'][i][at] = value
        return f

    u32 = lambda v: np.array(v, dtype=np.uint32)
    r = [('log2_ncos_small', field('log2_ncos', 3)), ('log2_ncos_big', field('log2_ncos', 9)), ('step_big', field('step', 2 ** 13 + 1)),
         ('nlevels_big', field('nlevels', 9)), ('first_big', field('first', 1041)), ('width_0', field('width', 0)), ('width_big', field('width', 2049)),
         ('profile_zero', field('profile', [0] * 64 + [9] * 192)),
         ('slowness_0', field('slowness', 0, 'timing')), ('slowness_big', field('slowness', 2 ** 24 + 1, 'timing')), ('bin_ticks_0', field('bin_ticks', 0, 'timing')),
         ('bin_ticks_big', field('bin_ticks', 2 ** 20 + 1, 'timing')), ('nbins_0', field('nbins', 0, 'timing')), ('nbins_big', field('nbins', 1025, 'timing')),
         ('ncand_0', arg(2, 0)), ('ncand_big', arg(2, 2 ** 20 + 1)), ('nchannels_big', arg(0, (2 ** 32 - 1) // 3 + 1)),
         ('channel_coordinate', coordinate(1, 4, 2 ** 23 + 1)), ('channel_coordinate_low', coordinate(1, 0, -2 ** 23 - 1)),
         ('cand_component', coordinate(3, 5, 2 ** 15 + 1)), ('cand_component_low', coordinate(3, 0, -2 ** 15 - 1)),
         ('vertex_coordinate', coordinate(7, 5, 2 ** 23 + 1)), ('vertex_coordinate_low', coordinate(7, 0, -2 ** 31)),
         ('offsets_start', arg(5, u32([1, 2, 3]))), ('offsets_descend', arg(5, u32([0, 3, 2]))), ('offsets_long', arg(5, u32([0, 65536, 65536]))),
         ('null_seeder', whole('seeder')), ('null_timing', whole('timing')), ('null_cand', arg(3, None)), ('null_offsets', arg(5, None)),
         ('null_tau0', arg(6, None)), ('null_vertex', arg(7, None)), ('null_bin', arg(8, None)), ('null_channel_pos', arg(1, None)),
         ('null_hit_channel', arg(9, None)), ('null_hit_weight', arg(11, None))]
    r += [('null_' + name, out(i)) for i, name in enumerate(OUTPUTS[:6])]
    return r


def refused_call(change):
    case = small_case()
    d = dict(seeder=dict(case['seeder']), timing=dict(case['timing']), args=list(case_arrays(case)), out=guarded(output_sizes(case)))
    change(d)
    return case, d


@pytest.mark.parametrize('name,change', refusals(), ids=[r[0] for r in refusals()])
def test_host_refusals_write_nothing(name, change):
    case, d = refused_call(change)
    assert host_call(d['seeder'], d['timing'], d['args'], d['out']) == CHROMA_ERR_INVALID, name
    assert all(a is None or np.all(a == SENTINEL) for a in d['out']), name


def test_the_small_call_is_valid_and_no_fits_write_nothing():
    case = small_case()
    rc, out, sizes = call_host(case)
    assert rc == 0
    check_outputs(case, out, sizes, 'host')
    # without times neither the timing nor tau0 nor the bins are needed
    args = list(case_arrays(case))
    args[6] = args[8] = args[10] = None
    out = guarded(sizes)
    assert host_call(case['seeder'], None, args, out) == 0
    check_outputs(dict(case, name='small_untimed', hit_time=None), out, sizes, 'host')
    args = list(case_arrays(case))
    args[4] = 0
    out = guarded(sizes)
    assert host_call(case['seeder'], case['timing'], args, out) == 0 and all(np.all(a == SENTINEL) for a in out)


# ---- the Python layer ----
def as_case(name, seeder, prepared):
    """a ``DirectionSeeder`` and its ``prepare`` as a case for the restatement"""
    s, t, v = prepared.struct, prepared.timing, seeder.vertex_seeder
    ints = lambda a: [int(x) for x in a]
    return dict(name=name, seeder=dict(log2_ncos=s.log2_ncos, step=s.step, nlevels=s.nlevels, first=s.first, width=s.width, profile=list(s.profile)),
                timing=dict(slowness=t.slowness, bin_ticks=t.bin_ticks, nbins=t.nbins), channel_pos=[tuple(ints(c)) for c in v.channel_pos],
                cand=[tuple(ints(c)) for c in seeder.cand], offsets=ints(prepared.offsets), tau0=ints(prepared.tau0), vertex=[tuple(ints(c)) for c in prepared.vertex],
                bin=ints(prepared.bin), hit_channel=ints(prepared.channel), hit_time=None if prepared.time is None else ints(prepared.time),
                hit_weight=ints(prepared.weight))


def python_layer_fixture(prompt_ns=(1.0, 2.5)):
    """25 channels, three fits (one without hits) of light from a point towards a cone, with times and charges: (the direction seeder,
    offsets, channel, t, w)"""
    rng = np.random.RandomState(11)
    positions = rng.uniform(-400.0, 400.0, size=(25, 3))
    vertex_seeder = VertexSeeder(positions, 190.0, bin_ns=0.8, spacing_mm=260.0, levels=3, ticks_per_bin=8, weights='npe')
    seeder = DirectionSeeder(vertex_seeder, profile=DirectionSeeder.cherenkov_profile(0.6, 0.2, fill=0.2, log2_ncos=5), log2_ncos=5, grid=3, levels=4,
                             prompt_ns=prompt_ns)
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


@pytest.mark.parametrize('prompt_ns', [(1.0, 2.5), None])
def test_fit_many_is_the_restatement_and_its_units(prompt_ns):
    seeder, offsets, channel, t, w = python_layer_fixture(prompt_ns)
    v = seeder.vertex_seeder
    seeds = v.fit_many(offsets, channel, t, w)
    fits = seeder.fit_many(seeds, offsets, channel, t, w, cos_hist=True)
    prepared = seeder.prepare(seeds, offsets, channel, t, w)
    assert prepared.vertex.tolist() == seeds.pos_int.tolist() and prepared.bin.tolist() == seeds.bin.tolist()
    assert (prepared.time is None) == (prompt_ns is None)
    if prompt_ns is not None:          # bins of 0.8 ns about the shape's peak: 2 before, 4 behind
        assert (seeder.first, seeder.width) == (v.peak - 2, 2 + 4 + 1) and seeder.first >= 0
    want = expected(as_case('python_layer_%s' % (prompt_ns is None), seeder, prepared))
    assert fits.dir_int.tolist() == want['best_dir'] and fits.score.tolist() == want['best_score'] and fits.cand.tolist() == want['best_cand']
    assert fits.inside.tolist() == want['inside'] and fits.outside.tolist() == want['outside'] and fits.level_score.tolist() == want['level_score']
    assert fits.cos_hist.tolist() == want['cos_hist'] and fits.nhits.tolist() == [25, 0, 17]
    assert isinstance(fits, DirFits) and len(fits) == 3 and fits.inside[0] > 0
    for k in range(3):
        length = math.sqrt(sum(x * x for x in want['best_dir'][k]))
        assert np.allclose(fits.dir[k], np.array(want['best_dir'][k]) / length, rtol=0, atol=1e-15)
    one = seeder.fit(seeds[0:1], channel[:25], t[:25], w[:25])
    assert one.dir_int.tolist() == want['best_dir'][:1] and one.score.tolist() == want['best_score'][:1] and one.cos_hist is None
    assert fits[2:3].dir_int.tolist() == want['best_dir'][2:] and fits[2:3].cos_hist.tolist() == want['cos_hist'][2:]
    vertices = to_vertices(seeds, fits, 'mu-', 500.0)
    assert len(vertices) == 3 and vertices[2].particle_name == 'mu-' and vertices[2].ke == 500.0 and vertices[2].t0 == seeds.t0[2]
    assert np.array_equal(vertices[2].pos, seeds.pos[2]) and np.array_equal(vertices[2].dir, fits.dir[2])
    with pytest.raises(ValueError):
        to_vertices(seeds[0:1], fits, 'mu-', 1.0)


def test_seeder_construction():
    v = VertexSeeder(np.array([[100.0, 0.0, 0.0], [-100.0, 0.0, 0.0]]), 200.0)
    s = DirectionSeeder(v)
    assert len(s.cand) == 6 * 12 * 12 and s.levels == 6 and s.log2_ncos == 6 and s.prompt is None
    assert s.step == math.floor(0.5 * (0.5 * math.pi / 12) * ONE + 0.5) == 1072
    lengths = np.sqrt((s.cand.astype(np.float64) ** 2).sum(axis=1))
    assert np.all(np.abs(lengths - ONE) < 2.0) and len({tuple(c) for c in s.cand.tolist()}) == 864
    assert np.array_equal(s.cand[:144, 0] > 0, np.ones(144, dtype=bool)) and np.array_equal(s.cand[144:288], s.cand[:144] * [-1, 1, 1])
    assert DirectionSeeder(v, grid=1).step == 2 ** 13 and len(DirectionSeeder(v, grid=1).cand) == 6
    profile = DirectionSeeder.cherenkov_profile(0.75, 0.05)
    assert len(profile) == 64 and max(profile) == 255 and profile[55] == profile[56] == 255 and profile[54] == profile[57] < 255 and profile[0] == 0 and profile[63] == 0          # (0.75 is the edge between bins 55 and 56)
    filled = DirectionSeeder.cherenkov_profile(0.75, 0.05, fill=0.25)
    assert filled[63] == 64 and filled[:56] == profile[:56] and min(filled[56:]) == 64
    assert len(DirectionSeeder.cherenkov_profile(0.5, 0.1, log2_ncos=4)) == 16
    assert DirectionSeeder.cherenkov_profile(0.75, 0.0) == [255 if k == 56 else 0 for k in range(64)]
    given = DirectionSeeder(v, directions=[[0.0, 0.0, 1.0], [0.6, 0.0, 0.8]], levels=0)
    assert given.cand.tolist() == [[0, 0, ONE], [9830, 0, 13107]]
    of = DirectionSeeder.of((0.75, 0.05, 0.25, 2), v)
    assert of.profile.tolist() == filled and of.levels == 2 and DirectionSeeder.of(of, v) is of
    assert DirectionSeeder.of(0.75, v).profile.tolist() == DirectionSeeder.cherenkov_profile(0.75, 0.1)
    for bad in (dict(log2_ncos=3), dict(levels=9), dict(profile=[0] * 64), dict(profile=[1] * 32), dict(directions=[[3.0, 0.0, 0.0]]), dict(prompt_ns=(-1.0, 1.0))):
        with pytest.raises(ValueError):
            DirectionSeeder(v, **bad)
    with pytest.raises(ValueError):
        DirectionSeeder.of(of, VertexSeeder(np.zeros((1, 3)), 200.0))


# ---- the ring ----
TRUE_AXIS = np.array([0.3, -0.5, 0.81]) / math.sqrt(0.3 ** 2 + 0.5 ** 2 + 0.81 ** 2)
RECORDED_DEGREES = 1.39          # the restatement's angle between the truth and the seeded axis (this file's docstring)


def covering_angle(seeder):
    """the farthest a direction lies from its nearest level-0 candidate, in degrees: taken at the corners of the cube-sphere
    grid's cells, where the distance to the cells' centres is greatest"""
    g = seeder.grid
    t = np.tan(np.arange(g + 1) / g * (0.5 * math.pi) - 0.25 * math.pi)
    v, u = np.meshgrid(t, t, indexing='ij')
    u, v, one = u.ravel(), v.ravel(), np.ones((g + 1) ** 2)
    corners = np.concatenate([np.stack(f, axis=1) for f in ((one, u, v), (-one, u, v), (u, one, v), (u, -one, v), (u, v, one), (u, v, -one))])
    corners /= np.sqrt((corners ** 2).sum(axis=1))[:, None]
    cand = seeder.cand.astype(np.float64)
    cand /= np.sqrt((cand ** 2).sum(axis=1))[:, None]
    return math.degrees(math.acos(float((corners @ cand.T).max(axis=1).min())))


def ring_fixture():
    n = 2000
    k = np.arange(n) + 0.5
    polar, azimuth = np.arccos(1.0 - 2.0 * k / n), math.pi * (1.0 + 5.0 ** 0.5) * k
    positions = 1000.0 * np.stack([np.sin(polar) * np.cos(azimuth), np.sin(polar) * np.sin(azimuth), np.cos(polar)], axis=1)
    vertex = np.array([123.4, -210.7, 88.8])
    seen = positions - vertex
    cosine = (seen @ TRUE_AXIS) / np.sqrt((seen ** 2).sum(axis=1))
    channel = np.nonzero(np.abs(cosine - 0.75) <= 0.05)[0]
    vertex_seeder = VertexSeeder(positions, 200.0)
    seeder = DirectionSeeder(vertex_seeder, profile=DirectionSeeder.cherenkov_profile(0.75, 0.05), grid=12, levels=6)
    pos_int = np.floor(vertex / vertex_seeder.unit + 0.5).astype(np.int32).reshape(1, 3)
    zero = np.zeros(1, dtype=np.uint32)
    seeds = SeedFits(pos_int * vertex_seeder.unit, np.zeros(1), zero, zero, zero, np.zeros((1, 1), dtype=np.uint32), zero, zero, pos_int)
    return seeder, seeds, channel


def angle_to_truth(direction):
    d = np.asarray(direction, dtype=np.float64)
    return math.degrees(math.acos(min(1.0, float(d @ TRUE_AXIS) / math.sqrt(float(d @ d)))))


def test_the_ring_is_seeded_within_the_grids_covering_angle():
    seeder, seeds, channel = ring_fixture()
    prepared = seeder.prepare(seeds, [0, len(channel)], channel)
    want = expected(as_case('ring', seeder, prepared))
    covering = covering_angle(seeder)
    restated = angle_to_truth(want['best_dir'][0])
    print('ring: %d hits, restated axis %s, %.3f degrees from the truth, covering angle %.3f degrees, level scores %s'
          % (len(channel), want['best_dir'][0], restated, covering, want['level_score'][0]))
    fit = seeder.fit(seeds, channel, cos_hist=True)
    assert fit.dir_int.tolist() == want['best_dir'] and fit.score.tolist() == want['best_score'] and fit.level_score.tolist() == want['level_score']
    assert fit.inside.tolist() == [len(channel)] and fit.outside.tolist() == [0] and fit.cos_hist.tolist() == want['cos_hist']
    assert 60 < len(channel) < 200 and 5.0 < covering < 5.5
    assert angle_to_truth(fit.dir[0]) < covering
    assert abs(restated - RECORDED_DEGREES) < 0.005          # (the record is the restatement's figure)
