"""SURVEY.md section 8 row a-20 on the device: the recursive-grid BVH builder as HIP kernels
(chroma_bvh_build_device, csrc/bvh_device.hip -- leaf boxes and Morton codes, device radix sort, parent unions per
layer, concatenate + offset, collapse; reference: chroma/cuda/bvh.cu:149-203,270-308,365-384,530-543 driven by
chroma/bvh/grid.py:11-95).  The node array must equal the host builder's and the NumPy restatement's bit for bit, and
the committed vectors of tests/golden/bvh_golden.json; and the device form of tools.argsort_direction."""
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def gpu():
    from chroma_amd import gpu as g
    ctx = g.create_cuda_context(0)
    yield g
    ctx.pop()


def _meshes():
    """The cases of tests/golden/bvh_golden.json (tools/gen_bvh_golden.py) + the 3 M-triangle C2-lite detector."""
    import sys
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    from gen_bvh_golden import CASES
    from chroma_amd import demo
    from chroma_amd.loader import create_geometry_from_obj
    for name, build in CASES.items():
        yield name, create_geometry_from_obj(build(), ).mesh
    yield 'lite', create_geometry_from_obj(demo.detector_lite()).mesh


def _sha(nodes):
    return hashlib.sha256(np.ascontiguousarray(nodes).tobytes()).hexdigest()


def test_device_builder_equals_the_host_builders(gpu):
    from chroma_amd.bvh.grid import make_recursive_grid_bvh
    golden = json.load(open(os.path.join(GOLDEN, 'bvh_golden.json')))
    for name, mesh in _meshes():
        for degree in (2, 3, 4):
            dev = make_recursive_grid_bvh(mesh, target_degree=degree, backend='device')
            host = make_recursive_grid_bvh(mesh, target_degree=degree, backend='native')
            assert len(dev.nodes) == len(host.nodes) and dev.layer_offsets == host.layer_offsets, (name, degree)
            assert np.array_equal(dev.nodes.view(np.uint32), host.nodes.view(np.uint32)), (name, degree)
            if len(mesh.triangles) < 500000:
                ref = make_recursive_grid_bvh(mesh, target_degree=degree, backend='numpy')
                assert np.array_equal(dev.nodes.view(np.uint32), ref.nodes.view(np.uint32)), (name, degree)
        if name in golden:                                        # the committed vectors (degree 3)
            dev = make_recursive_grid_bvh(mesh, backend='device')
            assert _sha(dev.nodes) == golden[name]['nodes_sha256'], name


def test_device_builder_is_the_default_with_a_gpu_and_refuses_bad_input(gpu):
    from chroma_amd import make, _lib
    from chroma_amd.geometry import Mesh
    from chroma_amd.bvh.grid import make_recursive_grid_bvh
    mesh = make.cube(10.0)
    a = make_recursive_grid_bvh(mesh, verbose=True)               # (prints "BVH (device)")
    b = make_recursive_grid_bvh(mesh, backend='native')
    assert np.array_equal(a.nodes.view(np.uint32), b.nodes.view(np.uint32))
    bad = Mesh(mesh.vertices, mesh.triangles.copy())
    bad.triangles[3, 1] = len(mesh.vertices)                     # a vertex index outside the mesh
    with pytest.raises(_lib.ChromaError):
        make_recursive_grid_bvh(bad, backend='device')


def test_direction_sort_is_argsort_direction_on_the_device(gpu, oracle_mod):
    """GPUPhotons.sort_by_direction == chroma_amd.tools.argsort_direction (chroma/tools.py:175-193) applied to every
    array of the set: codes non-decreasing, the same multiset of photons; equal to the NumPy order wherever the two
    arc functions give the same 16-bit angles (they differ in the last ulp for a few per million).  And exactly, row by
    row and with nothing left out: the stable order of the codes derived on the CPU from the contract's own acos and
    atan2 (test_gpu_photon_arrays.direction_codes)."""
    from chroma_amd.tools import argsort_direction
    from test_gpu_photon_arrays import direction_codes
    ph = oracle_mod.generate_bomb(200000, seed=3, id_base=0, wavelength_lo=300.0, wavelength_hi=700.0)
    gp = gpu.GPUPhotons(ph)
    gp.sort_by_direction()
    got = gp.get()

    def codes(d):
        maxint = 2 ** 16 - 1
        theta = (np.arccos(np.clip(d[:, 2], -1, 1)) / np.pi * maxint).astype(np.uint32)
        phi = ((np.arctan2(d[:, 1], d[:, 0]) / np.pi / 2.0 + 0.5) * maxint).astype(np.uint32)
        m = np.zeros(len(d), dtype=np.uint32)
        for i in range(16):
            bit = np.uint32(1 << i)
            m |= ((theta & bit) << np.uint32(i)) | ((phi & bit) << np.uint32(i + 1))
        return m
    c = codes(got.dir.astype(np.float64)).astype(np.int64)
    assert np.count_nonzero(np.diff(c) < 0) < 1e-4 * len(c)                      # sorted (up to last-ulp angle differences)
    order = argsort_direction(ph.dir)
    want = ph[order]
    same = (got.dir.view(np.uint32) == want.dir.view(np.uint32)).all(axis=1)
    assert same.mean() > 0.999
    # every photon is still there, whole: (wavelength, time, direction) rows as a multiset
    key_got = np.sort(np.ascontiguousarray(np.column_stack([got.wavelengths, got.dir, got.pol]).astype(np.float32)).view('V28').ravel())
    key_in = np.sort(np.ascontiguousarray(np.column_stack([ph.wavelengths, ph.dir, ph.pol]).astype(np.float32)).view('V28').ravel())
    assert np.array_equal(key_got, key_in)
    exact = ph[np.argsort(direction_codes(oracle_mod, ph.dir)[0], kind='stable')]
    for name in ('pos', 'dir', 'pol', 'wavelengths', 't', 'flags', 'last_hit_triangles', 'weights', 'evidx'):
        a, b = getattr(got, name), getattr(exact, name)
        differ = np.flatnonzero((a.view(np.uint32) != b.view(np.uint32)).reshape(len(a), -1).any(axis=1))
        assert len(differ) == 0, '%s: %d rows are not where the contract codes put them (first: row %d)' % (name, len(differ), differ[0])


# ---- the device builder at its size and run edges (the cases and the NumPy trees of tests/test_bvh.py) ------------------------
@pytest.fixture(scope='module')
def ctx(gpu):
    from chroma_amd.gpu import tools
    return tools._current


def _edge_case_names():
    from test_bvh import EDGE_CASES
    return list(EDGE_CASES)


@pytest.mark.parametrize('name', _edge_case_names())
def test_device_builder_on_the_edge_cases(ctx, name):
    """Bit for bit the host builder's and the NumPy restatement's nodes and layer bounds; and again on the same context,
    where every scratch array of the second build is a block the first one gave back to the pool."""
    from test_bvh import EDGE_CASES, native_tree, numpy_tree, assert_same_tree
    for degree in EDGE_CASES[name][2]:
        what = '%s, degree %d' % (name, degree)
        first = native_tree(name, degree, ctx=ctx)
        assert_same_tree(first, numpy_tree(name, degree), what + ': device against numpy')
        assert_same_tree(first, native_tree(name, degree), what + ': device against native')
        assert_same_tree(native_tree(name, degree, ctx=ctx), first, what + ': second device build')


def test_device_builder_refuses_a_bad_index_at_the_arrays_ends(ctx):
    """k_bvh_check_indices over 771 indices: the first and the last one.  The refused calls leave nothing behind: what the
    pool holds and what a good build takes from it afterwards are what they are without a refusal."""
    from chroma_amd import _lib
    from test_bvh import edge_case, native_tree, numpy_tree, assert_same_tree
    vertices, triangles, wc = edge_case('soup-257')

    def good_build():
        before = ctx.pool_stats()
        tree = native_tree('soup-257', 3, ctx=ctx)
        ctx.synchronize()
        after = ctx.pool_stats()
        return tree, (after[0], after[1] - before[1], after[2] - before[2])     # (parked bytes, blocks reused, blocks allocated)
    good_build()                                                               # (the pool now holds every block of this build)
    want, stats = good_build()
    assert stats[2] == 0, stats
    for row, slot in ((0, 0), (len(triangles) - 1, 2)):
        bad = triangles.copy()
        bad[row, slot] = len(vertices)
        with pytest.raises(_lib.ChromaError, match='outside the mesh'):
            _lib.bvh_build(vertices, bad, wc.world_origin, wc.world_scale, 3, ctx=ctx)
        ctx.synchronize()
    assert ctx.pool_stats()[0] == stats[0]
    got, stats_after = good_build()
    assert stats_after == stats
    assert_same_tree(got, want, 'after the refusals')
    assert_same_tree(got, native_tree('soup-257', 3), 'after the refusals: device against native')
    assert_same_tree(got, numpy_tree('soup-257', 3), 'after the refusals: device against numpy')


def test_device_builder_refuses_a_target_degree_below_two(ctx):
    from chroma_amd import _lib
    from chroma_amd.bvh.grid import make_recursive_grid_bvh
    from test_bvh import SAFE_FOR_ANY_DEGREE, BAD_DEGREES, _as_mesh, edge_case, native_tree, numpy_tree, assert_same_tree
    for name in SAFE_FOR_ANY_DEGREE:
        vertices, triangles, wc = edge_case(name)
        for degree in BAD_DEGREES:
            with pytest.raises(_lib.ChromaError, match='target_degree'):
                _lib.bvh_build(vertices, triangles, wc.world_origin, wc.world_scale, degree, ctx=ctx)
            with pytest.raises(ValueError, match='target_degree'):
                make_recursive_grid_bvh(_as_mesh(vertices, triangles), target_degree=degree, backend='device')
        assert_same_tree(native_tree(name, 2, ctx=ctx), numpy_tree(name, 2), name + ' after the refusals')


def test_device_builder_refuses_a_frame_that_cannot_quantise(ctx):
    from chroma_amd import _lib
    from chroma_amd.bvh.grid import make_recursive_grid_bvh, world_coords_for
    from test_bvh import unquantisable_meshes, _as_mesh, _words, edge_case, native_tree, numpy_tree, assert_same_tree
    for name, vertices, triangles in unquantisable_meshes():
        with pytest.raises(ValueError, match='no extent or has non-finite vertices'):
            make_recursive_grid_bvh(_as_mesh(vertices, triangles), backend='device')
        wc = world_coords_for(vertices)
        with pytest.raises(_lib.ChromaError, match='world_scale|world_origin'):
            _lib.bvh_build(vertices, triangles, wc.world_origin, wc.world_scale, 3, ctx=ctx)
    good_v, good_t, good = edge_case('soup-257')
    for scale in (0.0, -good.world_scale, np.nan, np.inf):
        with pytest.raises(_lib.ChromaError, match='world_scale'):
            _lib.bvh_build(good_v, good_t, good.world_origin, scale, 3, ctx=ctx)
    for value in (np.nan, np.inf, -np.inf):
        origin = good.world_origin.copy()
        origin[2] = value
        with pytest.raises(_lib.ChromaError, match='world_origin'):
            _lib.bvh_build(good_v, good_t, origin, good.world_scale, 3, ctx=ctx)
    assert_same_tree(native_tree('soup-257', 3, ctx=ctx), numpy_tree('soup-257', 3), 'soup-257 after the refusals')
    bvh = make_recursive_grid_bvh(_as_mesh(good_v, good_t), backend='device')
    assert np.array_equal(_words(bvh.nodes), numpy_tree('soup-257', 3)[0])


@pytest.mark.parametrize('name', ['identical-3376', 'soup-65537'])
def test_wide_tree_over_the_device_built_edge_trees(ctx, name):
    """The derived 8-wide tree, built on the device over DEVICE-built nodes that the test above has pinned, equals the host
    twin over the same nodes (tests/test_gpu_wide.py builds its soups' nodes on the device and compares them with nothing)."""
    from chroma_amd import _lib
    from chroma_amd.bvh.bvh import uint4
    from test_bvh import edge_case, native_tree, numpy_tree, assert_same_tree
    from test_gpu_wide import _host_levels, _same
    words, bounds = native_tree(name, 3, ctx=ctx)
    assert_same_tree((words, bounds), numpy_tree(name, 3), name)
    nodes = np.ascontiguousarray(words).view(uint4)[:, 0]
    nt = len(edge_case(name)[1])
    dev = _lib.wide_build(nodes, nt, ctx=ctx)
    _same(dev, _host_levels(nodes, nt), name)
    assert _lib.wide_validate(dev, nt), name
