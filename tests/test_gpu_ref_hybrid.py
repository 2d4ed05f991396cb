"""The hybrid render's kernels against the reference's OWN chroma/cuda/hybrid_render.cu, bit for bit, with the CPU oracle and the
Python restatements not in the chain.

The comparand is oracle/_ref/libchroma_ref_physics_contract.so alone: hybrid_render.cu compiled for the host
(oracle/ref_physics_driver.cc) with the transcendental calls of the sources it includes mapped onto include/chroma_math.h.  Nothing
here reads the reference tree.  tests/test_ref_hybrid_host.py holds the restatements to the same library on the CPU; this file
closes the triangle on the GPU: chroma_hybrid_lookup, _image and _pixels through the C entry points, on the guarded arrays of
tests/test_gpu_hybrid_edges.py (sentinels behind every array and in every row a call has no business in).

What the reference gives and the kernels must equal: the two tables of a launch from ZERO tables (on tables that hold values the
engine's per-key sum differs from fAtomicAdd by design, DESIGN.md 6, and test_gpu_hybrid_edges.py pins it), the draw counters, each
thread's own addition (row, table, cos_theta * xyz; the sample outputs triangle, side and cos), the image after two passes onto a lit
image, the key each image row names (triangle and side), the pixels.  The sample history has no counterpart in the reference and is
not compared here (NAN_ABORT for a zero or NaN direction is the engine's own bit).  A pixel channel that is NaN after the division
is left out, and only those: the reference's conversion of floorf(NaN) is undefined in a host build."""
import functools

import numpy as np
import pytest

import test_gpu_hybrid_edges as E
from test_gpu_hybrid_edges import (GUARD, PIXEL_SIZES, SCENES, SENTINEL, SIZES, XYZ, _bits, _ntri, _pixel_image, _start_counters,
                                   _start_table, call_image, call_lookup, call_pixels, ctx, device_scenes)  # noqa: F401  (fixtures)
from test_ref_hybrid_host import (ARMS, CHAIN_SCENE, IMAGE_SCENE, assert_same, bundle, chain_launch, coded_tables, live_threads, named_keys,
                                  pixel_mask, ref_image, ref_lookup, size_launch, zero_tables)

f32 = np.float32


def _have():
    import oracle
    return oracle.have_ref_hybrid()


pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not _have(), reason='oracle/_ref holds no hybrid render (it needs the reference tree at build time)')]


@functools.lru_cache(maxsize=None)
def reference_lookup(scene, nthreads, total, offset, ncounters, id_base=0):
    """The reference's launch from zero tables and _start_counters, computed once."""
    import oracle
    return ref_lookup(oracle, scene, nthreads, total, offset, _start_counters(ncounters), id_base=id_base, variant='contract')


def check_against_the_reference(a, reference, scene, n, counters, what):
    """Everything one lookup launch from zero tables must have done to its arrays by the reference's account, and nothing else."""
    nt = _ntri(scene)
    l1, l2, ctr, (tri, side, value) = reference
    after = a.after()
    adds = tri[:n] >= 0
    assert np.array_equal(after['triangle'][:n].view(np.int32), tri[:n]), '%s: the adding threads differ: %s' % (
        what, np.flatnonzero(after['triangle'][:n].view(np.int32) != tri[:n])[:8])
    assert np.array_equal(after['side'][:n], side[:n]), what + ': sides'
    cos = after['cos'][:n].view(f32)
    assert_same((cos[:, None] * np.asarray(XYZ, f32)[None, :]).astype(f32)[adds], value[:n][adds], what + ', cos_theta * xyz')
    for name in E.LOOKUP_SAMPLES:
        assert (after[name][n:] == SENTINEL).all(), '%s: %s was written past the last live thread' % (what, name)
    assert np.array_equal(after['counters'][:n], ctr[:n]), what + ': draw counters'
    assert np.array_equal(after['counters'][n:], a.before['counters'][n:]), what + ': a thread without a triangle drew, or a guard counter was written'
    assert np.array_equal(ctr[n:], np.asarray(counters)[n:])
    for name, w in (('lookup1', l1), ('lookup2', l2)):
        got = after[name][:3 * nt].reshape(nt, 3)
        bad = np.flatnonzero((got != _bits(w)).any(axis=1))
        assert len(bad) == 0, '%s: %s differs from the reference in %d rows, first triangle %d: %s, the reference %s' % (
            what, name, len(bad), bad[0], got[bad[0]].view(f32), w[bad[0]])
        assert (after[name][3 * nt:] == SENTINEL).all(), '%s: guard rows of %s were written' % (what, name)
    return int(adds.sum())


# ---- lookup -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('scene', sorted(SCENES))
def test_full_launches_are_the_reference(scene, ctx, device_scenes):
    g, packed, source, gg = device_scenes(scene)
    nt = len(g.mesh.triangles)
    counters = _start_counters(nt)
    a = call_lookup(ctx, gg, nt, nt, nt, 0, source, counters, zero_tables(nt))
    adds = check_against_the_reference(a, reference_lookup(scene, nt, nt, 0, nt), scene, nt, counters, '%s, full launch' % scene)
    assert adds >= {'room_sphere': 2049, 'room_sheet_mirror': 500}.get(scene, 10)


@pytest.mark.parametrize('arm', ARMS)
@pytest.mark.parametrize('n', SIZES)
def test_sizes_on_each_arm_of_the_cap_are_the_reference(n, arm, ctx, device_scenes):
    g, packed, source, gg = device_scenes('room_sheet_mirror')
    nt = len(g.mesh.triangles)
    nthreads, total, offset, ncounters = size_launch('room_sheet_mirror', n, arm)
    assert live_threads('room_sheet_mirror', nthreads, total, offset) == n
    counters = _start_counters(ncounters)
    a = call_lookup(ctx, gg, nt, nthreads, total, offset, source, counters, zero_tables(nt), id_base=129)
    reference = reference_lookup('room_sheet_mirror', nthreads, total, offset, ncounters, id_base=129)
    assert check_against_the_reference(a, reference, 'room_sheet_mirror', n, counters, '%d live threads by %s' % (n, arm)) > 0


def test_the_first_launches_of_the_chain_are_the_reference(ctx, device_scenes):
    """Launches 0 to 7 of test_ref_hybrid_host's chain on grey_stress (thin film, WLS, dichroic, detecting faces, grey walls), each
    from the counters the reference wrote in the one before."""
    import oracle
    g, packed, source, gg = device_scenes(CHAIN_SCENE)
    nt = len(g.mesh.triangles)
    adds = 0
    for k in range(8):
        counters, reference = chain_launch(oracle, k, 'contract')
        a = call_lookup(ctx, gg, nt, nt, nt, 0, source, counters, zero_tables(nt))
        adds += check_against_the_reference(a, reference, CHAIN_SCENE, nt, counters, 'grey_stress, launch %d of the chain' % k)
    assert adds >= 40


# ---- image ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,nlookup_calls', [('257', 3), ('scaled', 7), ('outside', 1)])
def test_image_two_passes_onto_a_lit_image_are_the_reference(name, nlookup_calls, ctx, device_scenes):
    import oracle
    g, packed, source, gg = device_scenes(IMAGE_SCENE)
    nt = len(g.mesh.triangles)
    o, d = bundle(name)
    n = len(o)
    tables = coded_tables(nt)
    counters, image = _start_counters(n), _start_table(n, 12)
    diffused = 0
    for k in range(2):
        what = 'bundle %s, pass %d' % (name, k)
        want, want_ctr = ref_image(oracle, name, counters, image, nlookup_calls, 'contract')
        dark, _ = ref_image(oracle, name, counters, np.zeros((n, 3), f32), nlookup_calls, 'contract')
        tri, side = named_keys(dark, nlookup_calls)
        a = call_image(ctx, gg, nt, o, d, counters, tables, image, nlookup_calls)
        after = a.after()
        assert_same(after['image'][:3 * n].view(f32).reshape(n, 3), want, what + ', image')
        assert (after['image'][3 * n:] == SENTINEL).all(), what + ': guard rows of the image were written'
        assert np.array_equal(after['counters'][:n], want_ctr), what + ': draw counters'
        assert (after['counters'][n:] == SENTINEL).all()
        assert np.array_equal(after['triangle'][:n].view(np.int32), tri), what + ': triangle against the key the image names'
        assert np.array_equal(after['side'][:n], side), what + ': side against the key the image names'
        for sample in E.IMAGE_SAMPLES:
            assert (after[sample][n:] == SENTINEL).all(), '%s: guard rows of %s were written' % (what, sample)
        a.assert_untouched(what, ('origins', 'directions', 'lookup1', 'lookup2'))
        diffused += int((tri >= 0).sum())
        counters, image = want_ctr, want
    assert diffused == 0 if name == 'outside' else diffused >= 100


# ---- pixels -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', PIXEL_SIZES)
def test_pixels_are_the_reference(n, ctx):
    import oracle
    image = _pixel_image(n + GUARD)
    want, left_out = oracle.ref_hybrid_pixels(image[:n], 3, variant='contract')
    assert np.array_equal(left_out, np.isnan(image[:n])), 'a channel other than the NaN ones was left out'
    mask = pixel_mask(left_out)
    a = call_pixels(ctx, n, image, 3)
    after = a.after()
    bad = np.flatnonzero((after['pixels'][:n] & mask) != (want & mask))
    assert len(bad) == 0, '%d of %d pixels differ, first %d: %08x, the reference %08x of %s' % (
        len(bad), n, bad[0], after['pixels'][bad[0]], want[bad[0]], image[bad[0]])
    assert (after['pixels'][n:] == SENTINEL).all(), 'guard pixels were written'
    a.assert_untouched('pixels', ('image',))
