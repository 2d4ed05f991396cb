"""The restatements of the hybrid render against the reference's OWN chroma/cuda/hybrid_render.cu, bit for bit, without a GPU.

oracle/_ref/libchroma_ref_physics_{libm,contract}.so hold hybrid_render.cu (to_diffuse, update_xyz_lookup, update_xyz_image,
process_image), compiled for the host by oracle/ref_physics_driver.cc over the stand-in headers of oracle/ref_shim.  The hybrid
kernels' other tests (test_gpu_hybrid_render.py, test_gpu_hybrid_edges.py, test_hybrid_host.py) compare with the project's own
restatements of that file: oracle_to_diffuse (oracle/chroma_oracle.c), oracle_lookup and oracle_image (test_gpu_hybrid_render.py),
hybrid_accumulate, hybrid_image_update and hybrid_pixels (chroma_amd/gpu/render.py).  Here those restatements are held to the text
they restate: the order of the two barycentric draws, 1.0f - a - b, the normal and the sign flip of cos_theta, the early return
after two draws, where to_diffuse tests REFLECT_DIFFUSE, which inside_to_outside survives the loop, xyz * lookup / nlookup_calls
as float3 operations, the clamp-then-floor of process_image.

Every comparison is made twice, reference(libm) against restatement(libm) and reference(contract) against restatement(contract),
bit for bit; two NaNs count as equal and there is no other tolerance.  The generator and the mapping of a word to a uniform are the
project's own contract on both sides (oracle/ref_shim/curand_kernel.h) and are not what these tests pin.

Three departures from the reference are deliberate and are not "fixed" here:
  - The engine sums one call's contributions per (triangle, side) in sample order and adds each sum once; the reference adds sample
    by sample (fAtomicAdd).  On tables that start from ZERO the two are the same float operations in the same order (the host
    driver runs thread 0 first, and 0 + c is exact), so every lookup launch here starts from zero tables; on tables that hold
    values the rules differ by design and test_gpu_hybrid_edges.py pins the engine's.
  - The engine's to_diffuse sets NAN_ABORT in the sample history of a zero or NaN direction.  The reference has no such check
    and exposes no history; image and counters must still agree for those rays, and do.  (The host build of the reference runs
    intersect_mesh on a NaN direction without anything undefined: mesh.h and intersect.h only compare and do arithmetic on
    the NaNs, no float becomes an integer or an index, and the walk ends without a hit.)
  - NaN pixels: process_image converts floorf(NaN) to unsigned, undefined in a host build, 0 on the device.  Channels that are NaN
    after the division are left out of the reference comparison (oracle.ref_hybrid_pixels hands them over as 0.0), and only
    those; hybrid_pixels keeps pinning them ("NaN to 0").
One more difference is not the kernel's but its caller's: update_xyz_lookup fetches triangle offset + k for every thread below
total_threads and the camera passes the triangle count there (chroma/camera.py:213-217).  The engine caps by the triangle count
itself; a launch told of more threads than triangles meets the reference as the launch with total_threads = the triangle count.

The history is the one sample output the reference does not expose: the surface models a chain of launches went through are read
from the restatement, on launches whose records the same test has just shown equal to the reference's.

Preconditions (evaluated on the REFERENCE's result alone, so that no case passes empty), as measured when this was written, the
same in both builds:
  room               16 threads add
  room_sheet_mirror  529 of 530 threads add, the longest key run 265 records      (floors: 500 and 256)
  room_sphere        2157 of 4432 threads add, the longest key run 2142 records   (floor: more than 2048, eight blocks of k_hybrid_reduce)
  sheet_mirror32     17 threads add, 15 do not                                    (floors: 10 and 10)
  grey_stress        12 of 48 threads add; its chain of 64 launches: 696 threads add of 1129 that reach their own triangle, and
                     the diffusing samples carry SURFACE_TRANSMIT, SURFACE_REEMIT, REFLECT_SPECULAR, RAYLEIGH_SCATTER, BULK_REEMIT
                     and REFLECT_DIFFUSE among them                               (floor: 500)

The tests skip only where oracle/_ref holds no hybrid render (no reference tree at build time, or libraries built before this)."""
import numpy as np
import pytest

from chroma_amd import event
from chroma_amd.gpu.render import hybrid_image_update, hybrid_pixels
import test_gpu_hybrid_edges as E
from test_gpu_hybrid_edges import (BIG_ID, OUTSIDE_SOURCE, SCENES, SEED, SIZES, WAVELENGTH, XYZ, _ntri, _pixel_image, _start_counters,
                                   _start_table, broken_bundle, camera_bundle, outside_bundle, scaled_bundle, want_image, want_lookup)

f32 = np.float32
VARIANTS = ('libm', 'contract')
ARMS = ('nthreads', 'total', 'ntriangles')
SIZES_OFFSET = 7                                  # the non-zero first triangle of the size launches
CHAIN_SCENE, CHAIN_LENGTH = 'grey_stress', 64
CHAIN_BITS = ('SURFACE_TRANSMIT', 'SURFACE_REEMIT', 'REFLECT_SPECULAR', 'RAYLEIGH_SCATTER', 'BULK_REEMIT', 'REFLECT_DIFFUSE')
NLOOKUP_CALLS = (1, 3, 7)
IMAGE_SCENE = 'room_sheet_mirror'


@pytest.fixture(scope='module')
def ref(oracle_mod):
    """The oracle module, once both physics libraries hold the reference's hybrid render."""
    if not oracle_mod.have_ref_hybrid():
        pytest.skip('oracle/_ref holds no hybrid render (it needs the reference tree at build time)')
    return oracle_mod


# ---- comparing ------------------------------------------------------------------------------------------------------------------
def same(a, b):
    """Elementwise: the same bits, or two NaNs."""
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    assert a.shape == b.shape
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def assert_same(got, want, what):
    ok = same(got, want)
    bad = np.argwhere(~ok)
    assert ok.all(), '%s: %d of %d values differ, first at %s: %r, wanted %r' % (
        what, len(bad), ok.size, bad[0].tolist(), np.asarray(got)[tuple(bad[0])], np.asarray(want)[tuple(bad[0])])


def zero_tables(ntri):
    return np.zeros((ntri, 3), f32), np.zeros((ntri, 3), f32)


# ---- lookup launches --------------------------------------------------------------------------------------------------------------
def size_launch(scene, n, arm):
    """(nthreads, total_threads, offset, ncounters) that leave n live threads from a non-zero first triangle, capped by `arm` of
    min(offset + nthreads, total_threads, ntriangles)."""
    nt = _ntri(scene)
    if arm == 'nthreads':
        return n, nt, SIZES_OFFSET, n
    if arm == 'total':
        return n + 40, SIZES_OFFSET + n, SIZES_OFFSET, n + 45
    return n + 40, nt + 100, nt - n, n + 40                     # 'ntriangles': a chunk that runs past the last triangle


def ref_lookup(oracle_mod, scene, nthreads, total, offset, counters, max_steps=10, source=None, id_base=0, variant='contract'):
    """The reference's launch from zero tables.  total_threads is capped by the triangle count, as the camera passes it (see
    the module docstring).  Returns (lookup1, lookup2, counters, (triangle, side, value))."""
    g, packed, src = SCENES[scene]()
    nt = len(g.mesh.triangles)
    return oracle_mod.ref_hybrid_lookup(packed, SEED, id_base, counters, nthreads, min(total, nt), offset, src if source is None else source,
                                        WAVELENGTH, XYZ, *zero_tables(nt), max_steps=max_steps, variant=variant)


def live_threads(scene, nthreads, total, offset):
    return max(0, min(offset + nthreads, total, _ntri(scene)) - offset)


def check_lookup(oracle_mod, scene, nthreads, total, offset, counters, variant, max_steps=10, source=None, id_base=0):
    """One launch: tables from zero, counters and per-thread records of the reference against the restatement.  Returns
    (the restatement's Want, the reference's records)."""
    nt = _ntri(scene)
    n = live_threads(scene, nthreads, total, offset)
    counters = np.asarray(counters, np.uint32)
    what = '%s (%s): %d threads of %d from triangle %d, max_steps %d' % (scene, variant, nthreads, total, offset, max_steps)
    l1, l2, ctr, (tri, side, value) = ref_lookup(oracle_mod, scene, nthreads, total, offset, counters, max_steps, source, id_base, variant)
    want = want_lookup(oracle_mod, scene, n, offset, counters, max_steps=max_steps, source=source, id_base=id_base, variant=variant)
    w1, w2 = want.add_to(*zero_tables(nt))
    assert_same(l1, w1, what + ', lookup1')
    assert_same(l2, w2, what + ', lookup2')
    assert np.array_equal(ctr[:n], want.ctr), '%s: draw counters differ for threads %s' % (what, np.flatnonzero(ctr[:n] != want.ctr)[:8])
    assert np.array_equal(ctr[n:], counters[n:]), what + ': a thread without a triangle drew'
    assert np.array_equal(tri[:n], want.tri), '%s: the adding threads differ: %s' % (what, np.flatnonzero(tri[:n] != want.tri)[:8])
    assert (tri[n:] == -1).all(), what + ': a thread without a triangle added'
    assert np.array_equal(side[:n], want.side), what + ': sides'
    contrib = (want.cos[:, None] * np.asarray(XYZ, f32)[None, :]).astype(f32)
    contrib[want.tri < 0] = 0
    assert_same(value[:n], contrib, what + ', cos_theta * xyz')
    return want, (tri, side, value)


def key_runs(tri, side):
    """{(triangle, side): records} of the reference's per-thread records."""
    keys, counts = np.unique(2 * tri[tri >= 0].astype(np.int64) + side[tri >= 0], return_counts=True)
    return dict(zip(keys.tolist(), counts.tolist()))


FULL_FLOORS = {                      # scene -> (threads that add at least, threads that do not at least, longest key run at least)
    'room': (16, 0, 1), 'room_sheet_mirror': (500, 0, 256), 'room_sphere': (2049, 0, 2049), 'sheet_mirror32': (10, 10, 1), 'grey_stress': (1, 1, 1)}


@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('scene', sorted(SCENES))
def test_full_launches_at_max_steps_0_1_and_10(ref, scene, variant):
    nt = _ntri(scene)
    c0 = _start_counters(nt)
    for max_steps in (10, 1, 0):
        want, (tri, side, value) = check_lookup(ref, scene, nt, nt, 0, c0, variant, max_steps=max_steps)
        if max_steps == 10:
            runs = key_runs(tri, side)
            adds, longest = int((tri >= 0).sum()), max(runs.values())
            print('%s (%s): %d of %d threads add, longest key run %d' % (scene, variant, adds, nt, longest))
            floor_add, floor_idle, floor_run = FULL_FLOORS[scene]
            assert adds >= floor_add and nt - adds >= floor_idle and longest >= floor_run, (adds, nt - adds, longest)
        if max_steps == 0:
            assert (tri == -1).all() and not value.any()


@pytest.mark.parametrize('variant', VARIANTS)
def test_the_room_from_outside(ref, variant):
    want, (tri, side, value) = check_lookup(ref, 'room', 16, 16, 0, _start_counters(16), variant, source=OUTSIDE_SOURCE)
    assert 0 < (tri >= 0).sum() < 16 and (side[tri >= 0] == 0).all()               # the near wall, seen against its normal: lookup2


@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('arm', ARMS)
@pytest.mark.parametrize('n', SIZES)
def test_sizes_from_a_non_zero_offset_on_each_arm_of_the_cap(ref, n, arm, variant):
    nthreads, total, offset, ncounters = size_launch('room_sheet_mirror', n, arm)
    assert offset > 0 and live_threads('room_sheet_mirror', nthreads, total, offset) == n
    want, (tri, side, value) = check_lookup(ref, 'room_sheet_mirror', nthreads, total, offset, _start_counters(ncounters), variant, id_base=129)
    assert (tri >= 0).any()


@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('scene,n', [('grey_stress', 48), ('room_sheet_mirror', 129)])
def test_stream_ids_past_two_to_the_32(ref, scene, n, variant):
    want, (tri, side, value) = check_lookup(ref, scene, n, _ntri(scene), 0, _start_counters(n), variant, id_base=BIG_ID)
    low, _ = check_lookup(ref, scene, n, _ntri(scene), 0, _start_counters(n), variant, id_base=BIG_ID % 2 ** 32)
    assert (tri >= 0).any() and not same(want.cos, low.cos).all()                    # the high word of the id is part of the stream


def chain_launch(oracle_mod, k, variant='contract'):
    """(counters before, reference result) of launch k of the chain: 64 full launches on grey_stress from zero tables, launch 0
    from zero counters, each continuing the counters the reference wrote in the one before."""
    key = ('chain', k, variant)
    if key not in E._memo:
        nt = _ntri(CHAIN_SCENE)
        counters = np.zeros(nt, np.uint32) if k == 0 else chain_launch(oracle_mod, k - 1, variant)[1][2]
        E._memo[key] = (counters, ref_lookup(oracle_mod, CHAIN_SCENE, nt, nt, 0, counters, variant=variant))
    return E._memo[key]


@pytest.mark.parametrize('variant', VARIANTS)
def test_every_surface_model_in_a_chain_of_64_launches(ref, variant):
    nt = _ntri(CHAIN_SCENE)
    adds = mine = union = 0
    counters = np.zeros(nt, np.uint32)
    for k in range(CHAIN_LENGTH):
        assert np.array_equal(chain_launch(ref, k, variant)[0], counters)
        want, (tri, side, value) = check_lookup(ref, CHAIN_SCENE, nt, nt, 0, counters, variant)
        adds += int((tri >= 0).sum())
        mine += int(want.mine.sum())
        if (tri >= 0).any():
            union |= int(np.bitwise_or.reduce(want.hist[tri >= 0]))       # of launches whose records were just shown equal
        assert (want.ctr > counters).all()
        counters = want.ctr
    print('grey_stress chain (%s): %d threads add of %d that reach their triangle; bits %s' % (
        variant, adds, mine, [b for b in CHAIN_BITS if union & getattr(event, b)]))
    assert adds >= 500, adds
    missing = [b for b in CHAIN_BITS if not union & getattr(event, b)]
    assert not missing, 'no diffusing sample of the chain went through %s' % missing


# ---- image ------------------------------------------------------------------------------------------------------------------------
def coded_tables(ntri):
    """lookup1 / lookup2 whose entries are all distinct small integers: 1 + 6 t + c in lookup1, 4 + 6 t + c in lookup2."""
    base = f32(1) + f32(6) * np.arange(ntri, dtype=f32)[:, None] + np.arange(3, dtype=f32)[None, :]
    return base.astype(f32), (base + f32(3)).astype(f32)


def named_keys(image, nlookup_calls, xyz=XYZ):
    """(triangle or -1, side) that each row of an image names, the image being ONE pass from zero over coded_tables: the row is
    xyz * code / nlookup_calls in float32, two roundings of relative 6e-8 each on a code below 2^12, so the nearest integer to
    row * nlookup_calls / xyz in float64 is the code."""
    image = np.asarray(image, f32).reshape(-1, 3)
    lit = image.any(axis=1)
    code = np.rint(image.astype(np.float64) * nlookup_calls / np.asarray(xyz, f32).astype(np.float64)[None, :]).astype(np.int64)
    assert (code[lit, 1] == code[lit, 0] + 1).all() and (code[lit, 2] == code[lit, 0] + 2).all(), 'a row names no single key'
    assert (lit[:, None] == (image != 0)).all(), 'a row is lit in part'
    k = code[:, 0] - 1
    assert np.isin(k[lit] % 6, (0, 3)).all()
    tri = np.where(lit, k // 6, -1).astype(np.int32)
    side = np.where(lit & (k % 6 == 0), 1, 0).astype(np.uint32)
    return tri, side


def bundle(name):
    if name == 'outside':
        return outside_bundle()
    if name == 'scaled':
        return scaled_bundle()[:2]
    if name == 'broken':
        return broken_bundle()
    return camera_bundle(int(name))


BUNDLES = tuple(str(n) for n in SIZES) + ('outside', 'scaled', 'broken')


def ref_image(oracle_mod, name, counters, image, nlookup_calls, variant='contract', max_steps=10):
    g, packed, _ = SCENES[IMAGE_SCENE]()
    o, d = bundle(name)
    l1, l2 = coded_tables(len(g.mesh.triangles))
    return oracle_mod.ref_hybrid_image(packed, SEED, 0, counters, o, d, WAVELENGTH, XYZ, l1, l2, image, nlookup_calls, max_steps=max_steps,
                                       variant=variant)


@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('nlookup_calls', NLOOKUP_CALLS)
@pytest.mark.parametrize('name', BUNDLES)
def test_image_two_passes_onto_a_lit_image(ref, name, nlookup_calls, variant):
    o, d = bundle(name)
    n = len(o)
    l1, l2 = coded_tables(_ntri(IMAGE_SCENE))
    counters, image = _start_counters(n), _start_table(n, 12)
    diffused = 0
    for k in range(2):
        what = 'bundle %s (%s), nlookup_calls %d, pass %d' % (name, variant, nlookup_calls, k)
        tri, side, hist, ctr = want_image(ref, IMAGE_SCENE, o, d, counters, variant=variant)
        got, got_ctr = ref_image(ref, name, counters, image, nlookup_calls, variant)
        assert_same(got, hybrid_image_update(image.copy(), tri, side, l1, l2, XYZ, nlookup_calls), what + ', image')
        assert np.array_equal(got_ctr, ctr), what + ': draw counters'
        # the key each ray read, from the reference alone: the same pass onto a dark image
        dark, dark_ctr = ref_image(ref, name, counters, np.zeros((n, 3), f32), nlookup_calls, variant)
        named_tri, named_side = named_keys(dark, nlookup_calls)
        assert np.array_equal(named_tri, tri) and np.array_equal(named_side, side), what + ': the keys the image names'
        assert np.array_equal(dark_ctr, ctr)
        diffused += int((named_tri >= 0).sum())
        counters, image = got_ctr, got
    if name == 'outside':
        assert diffused == 0
    else:
        assert diffused > 0 and (n < 63 or (len(set(named_tri.tolist())) >= 5 and set(named_side.tolist()) == {0, 1}))
    if name == 'broken':
        for ray in (E.ZERO_RAY, E.NAN_RAY):
            assert named_tri[ray] == -1 and hist[ray] == (event.NO_HIT | event.NAN_ABORT)    # the bit is the engine's; image and counter agree


# ---- pixels -----------------------------------------------------------------------------------------------------------------------
def pixel_mask(left_out):
    """The bits of a pixel that are compared: alpha, and the eight bits of every channel that is not left out."""
    keep = ~np.asarray(left_out, bool)
    return (np.uint32(0xFF000000) | (keep[:, 0] * np.uint32(0xFF0000)) | (keep[:, 1] * np.uint32(0xFF00)) | (keep[:, 2] * np.uint32(0xFF))).astype(np.uint32)


@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('nimages', [1, 3, 255])
def test_pixels_clamp_then_floor(ref, nimages, variant):
    image = _pixel_image(257 + E.GUARD)
    got, left_out = ref.ref_hybrid_pixels(image, nimages, variant=variant)
    with np.errstate(invalid='ignore', over='ignore'):
        nan = np.isnan(image / f32(nimages))
    assert np.array_equal(left_out, nan) and np.array_equal(nan, np.isnan(image)), 'a channel other than the NaN ones was left out'
    assert 0 < nan.sum() < 0.05 * nan.size
    mask = pixel_mask(left_out)
    assert np.count_nonzero(mask & 0xFF0000) + np.count_nonzero(mask & 0xFF00) + np.count_nonzero(mask & 0xFF) == nan.size - nan.sum()
    want = hybrid_pixels(image, nimages)
    bad = np.flatnonzero((got & mask) != (want & mask))
    assert len(bad) == 0, '%d of %d pixels differ, first %d: %08x, hybrid_pixels %08x of %s' % (
        len(bad), len(image), bad[0], got[bad[0]], want[bad[0]], image[bad[0]])
    assert (got >> 24 == 0xFF).all() and len(np.unique((got >> 16) & 0xFF)) >= 10
