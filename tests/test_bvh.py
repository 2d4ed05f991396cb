"""BVH data model (port of the reference's test/test_bvh.py) and the two builders."""
import numpy as np
import pytest

from chroma_amd.bvh import (BVH, BVHLayerSlice, WorldCoords, OutOfRangeError, uint4, unpack_nodes,
                            make_recursive_grid_bvh, CHILD_BITS)
from chroma_amd import make as M


class TestWorldCoords:
    coords = WorldCoords([-1, -1, -1], 0.1)

    def test_fixed_to_world(self):
        np.testing.assert_array_max_ulp(self.coords.fixed_to_world([0, 1, 100]), [-1.0, -0.9, 9.0], dtype=np.float32)

    def test_world_to_fixed(self):
        np.testing.assert_array_equal(self.coords.world_to_fixed([-1.0, -0.9, 9.0]), [0, 1, 100])

    def test_arrays(self):
        f = [[0, 1, 100], [20, 40, 60], [210, 310, 410]]
        w = [[-1.0, -0.9, 9.0], [1.0, 3.0, 5.0], [20.0, 30.0, 40.0]]
        np.testing.assert_array_max_ulp(self.coords.fixed_to_world(f), w, dtype=np.float32)
        np.testing.assert_array_equal(self.coords.world_to_fixed(w), f)

    def test_out_of_range(self):
        with pytest.raises(OutOfRangeError):
            self.coords.world_to_fixed([-2.0, 0.0, 0.0])
        with pytest.raises(OutOfRangeError):
            self.coords.world_to_fixed([0.0, 1e9, 0.0])


def hand_built_bvh():
    """3-layer binary tree as in test/test_bvh.py:create_bvh, in the current leaf convention
    (nchild == 0 marks a leaf)."""
    wc = WorldCoords(np.array([-1.0, -1.0, -1.0]), 0.1)
    bounds = [0, 1, 3, 7]
    nodes = np.empty(bounds[-1], dtype=uint4)
    for i, (lo, hi) in enumerate([(0, 1), (1, 2), (2, 3), (3, 4)]):
        n = nodes[3 + i]
        nodes['x'][3 + i] = lo | (hi << 16); nodes['y'][3 + i] = lo | (hi << 16); nodes['z'][3 + i] = lo | (hi << 16)
        nodes['w'][3 + i] = i
    for p, (c0, lo, hi) in zip((1, 2), ((3, 0, 2), (5, 2, 4))):
        nodes['x'][p] = nodes['y'][p] = nodes['z'][p] = lo | (hi << 16)
        nodes['w'][p] = (2 << CHILD_BITS) | c0
    nodes['x'][0] = nodes['y'][0] = nodes['z'][0] = 0 | (4 << 16)
    nodes['w'][0] = (2 << CHILD_BITS) | 1
    return BVH(wc, nodes, bounds[:-1])


def test_bvh_container():
    bvh = hand_built_bvh()
    assert len(bvh) == 7 and bvh.layer_count() == 3
    assert [len(bvh.get_layer(i)) for i in range(3)] == [1, 2, 4]
    u = unpack_nodes(bvh.nodes)
    assert u['nchild'].tolist() == [2, 2, 2, 0, 0, 0, 0] and u['child'][:3].tolist() == [1, 3, 5]
    assert u['xhi'][0] == 4 and u['xlo'][0] == 0
    layer = bvh.get_layer(2)
    assert isinstance(layer, BVHLayerSlice)
    assert layer.area_fixed() == 4 * 6.0 and layer.area() == pytest.approx(4 * 6.0 * 0.01, rel=1e-6)
    assert bvh.get_layer(0).area_fixed() == 6 * 16.0


def _ranges(first, count):
    """The concatenation of arange(f, f + c) over the pairs of (first, count)."""
    first, count = np.asarray(first, dtype=np.int64), np.asarray(count, dtype=np.int64)
    starts = np.cumsum(count) - count
    return np.repeat(first, count) + (np.arange(int(count.sum()), dtype=np.int64) - np.repeat(starts, count))


def check_tree_invariants(bvh, ntriangles):
    nodes = bvh.nodes
    u = unpack_nodes(nodes)
    n = len(nodes)
    assert bvh.layer_offsets[0] == 0 and u['nchild'].max() <= 15
    inner = np.flatnonzero(u['nchild'] > 0)
    first = u['child'][inner].astype(np.int64)
    cnt = u['nchild'][inner].astype(np.int64)
    assert (first > inner).all() and (first + cnt <= n).all()
    # every child box lies inside its parent's box
    parent_of = np.repeat(inner, cnt)
    child = _ranges(first, cnt)
    for ax in 'xyz':
        assert (u[ax + 'lo'][child] >= u[ax + 'lo'][parent_of]).all()
        assert (u[ax + 'hi'][child] <= u[ax + 'hi'][parent_of]).all()
    # every triangle sits in exactly one REACHABLE leaf
    reach = np.zeros(n, dtype=bool)
    frontier = np.array([0])
    seen_tri = []
    while len(frontier):
        reach[frontier] = True
        leaves = frontier[u['nchild'][frontier] == 0]
        seen_tri.append(u['child'][leaves])
        inn = frontier[u['nchild'][frontier] > 0]
        frontier = _ranges(u['child'][inn].astype(np.int64), u['nchild'][inn].astype(np.int64))
    tri = np.sort(np.concatenate(seen_tri))
    assert np.array_equal(tri, np.arange(ntriangles))


@pytest.mark.parametrize('mesh_fn', [lambda: M.box(100, 100, 100), lambda: M.sphere(1000.0, 24), lambda: M.torus(5, 20, 12, 8)])
def test_builders_agree_and_tree_is_valid(mesh_fn):
    mesh = mesh_fn()
    a = make_recursive_grid_bvh(mesh, backend='numpy')
    b = make_recursive_grid_bvh(mesh, backend='native')
    assert np.array_equal(a.nodes, b.nodes) and a.layer_offsets == b.layer_offsets
    assert a.world_coords.world_scale == b.world_coords.world_scale
    check_tree_invariants(b, len(mesh.triangles))


def test_tiny_detector_bvh(tiny_geometry):
    bvh = tiny_geometry.bvh
    mesh = tiny_geometry.mesh
    assert len(mesh.triangles) == 389568
    assert bvh.layer_count() == 11 and len(bvh.get_layer(10)) == 389568
    assert bvh.world_coords.world_scale == pytest.approx(0.0762963, rel=1e-5)
    ref = make_recursive_grid_bvh(mesh, backend='numpy')
    assert np.array_equal(ref.nodes, bvh.nodes)
    check_tree_invariants(bvh, len(mesh.triangles))
    # leaves contain their triangles (padded by one quantum)
    u = unpack_nodes(bvh.get_layer(10).nodes)
    tri = mesh.vertices[mesh.triangles[u['child']]]
    lo = bvh.world_coords.fixed_to_world(np.column_stack([u['xlo'], u['ylo'], u['zlo']]))
    hi = bvh.world_coords.fixed_to_world(np.column_stack([u['xhi'], u['yhi'], u['zhi']]))
    assert (tri.min(axis=1) >= lo - 1e-3).all() and (tri.max(axis=1) <= hi + 1e-3).all()


def test_single_triangle_and_degenerate_inputs():
    from chroma_amd.geometry import Mesh
    one = Mesh(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=float), [[0, 1, 2]])
    for backend in ('numpy', 'native'):
        bvh = make_recursive_grid_bvh(one, backend=backend)
        assert len(bvh) == 1 and bvh.nodes['w'][0] == 0
    with pytest.raises(Exception):
        make_recursive_grid_bvh(Mesh(np.zeros((3, 3)), np.zeros((0, 3), dtype=int)), backend='native')


@pytest.mark.parametrize('case', ['tiny', 'box100', 'cube1000', 'sphere100_16'])
def test_bvh_golden_layers_and_node_hash(case):
    """SURVEY.md 8(c) golden 4: the full list of layer sizes, the world frame and the SHA-256 of the packed node
    array against the committed tests/golden/bvh_golden.json (tools/gen_bvh_golden.py), for BOTH builders."""
    import hashlib
    import json
    import os
    import sys
    from conftest import GOLDEN, ROOT
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    from gen_bvh_golden import CASES
    from chroma_amd.geometry import Geometry, Solid, Mesh
    from chroma_amd.loader import create_geometry_from_obj
    want = json.load(open(os.path.join(GOLDEN, 'bvh_golden.json')))[case]
    geo = create_geometry_from_obj(CASES[case]())
    for backend in ('native', 'numpy'):
        bvh = make_recursive_grid_bvh(geo.mesh, backend=backend)
        nodes = np.ascontiguousarray(bvh.nodes).view(np.uint32).reshape(-1, 4)
        lo = [int(x) for x in bvh.layer_offsets]
        assert [b - a for a, b in zip(lo, lo[1:] + [len(nodes)])] == want['layer_sizes'], backend
        assert len(geo.mesh.triangles) == want['ntriangles'] and len(nodes) == want['nnodes']
        assert float(np.float32(bvh.world_coords.world_scale)) == want['world_scale']
        assert [float(np.float32(x)) for x in bvh.world_coords.world_origin] == want['world_origin']
        assert hashlib.sha256(nodes.tobytes()).hexdigest() == want['nodes_sha256'], backend


# ---- the builders at their size and run edges --------------------------------------------------------------------------------
# Triangle soups and degenerate meshes as plain arrays (no Mesh: it removes duplicates and null triangles), shared with
# tests/test_gpu_bvh.py, where the device builder is held against the same NumPy trees.  The device code finds run starts,
# the cuts of runs longer than 15 and the parents' first children with a histogram pass and two scans, the host builder and
# the NumPy restatement with a loop over the sorted codes: the sizes sit on the 256-thread block edge of every kernel, on
# 15 x 256, on the host builder's 65536 threshold for its threaded count, and (the large soup) beyond the 4096-block grid
# cap of the histogram kernel.
import functools
import types

SOUP_SIZES = (1, 2, 3, 15, 16, 17, 255, 256, 257, 511, 513, 3840, 3841, 65535, 65536, 65537)
IDENTICAL_COUNTS = (15, 16, 225, 226, 3376)
LARGE_SOUP = 2 ** 20 + 257
LARGE_TRIPLED = 349611                  # 3 x 349611 + 1 = 2^20 + 258 leaves
EDGE_DEGREES = (2, 3, 16)


def _own_vertices(name, tri):
    """(name, vertices, triangles) of an (n, 3, 3) array: every triangle has its own three vertices."""
    n = len(tri)
    return name, np.ascontiguousarray(tri.reshape(-1, 3), dtype=np.float32), np.arange(3 * n, dtype=np.uint32).reshape(-1, 3)


def _soup(n, seed):
    """The recipe of tests/test_gpu_wide.py: centres uniform in +-50, vertices normal(0, 6) around them; from 64 triangles on
    a block of n // 8 identical triangles in the middle and the last n // 16 triangles in the plane x = 1."""
    rng = np.random.default_rng(seed)
    centre = rng.uniform(-50, 50, size=(n, 1, 3)).astype(np.float32)
    tri = centre + rng.normal(0, 6, size=(n, 3, 3)).astype(np.float32)
    if n >= 64:
        tri[n // 2:n // 2 + n // 8] = tri[n // 2]
        tri[n - n // 16:, :, 0] = 1.0
    return tri


def soup_case(n, seed):
    return _own_vertices('soup-%d' % n, _soup(n, seed))


def identical_case(m):
    """m copies of one triangle: every layer is ONE run, cut at 15, through several layers; 16 and 226 leave a one-child
    remainder that the collapse must lift."""
    one = np.array([[0, 0, 0], [10, 0, 0], [0, 10, 5]], dtype=np.float32)
    return _own_vertices('identical-%d' % m, np.repeat(one[None], m, axis=0))


def planar_case():
    tri = _soup(5000, 117)
    tri[:, :, 2] = 0.0                                         # a whole axis without extent
    return _own_vertices('planar', tri)


def collinear_case():
    tri = _soup(5000, 118)
    tri[:, :, 1:] = 0.0                                        # two axes without extent
    return _own_vertices('collinear', tri)


def reversed_sphere_case():
    """Shared vertices, and the triangle list back to front: equal codes must keep TRIANGLE order through the sort."""
    mesh = M.sphere(100.0, 40)
    return ('sphere-reversed', np.ascontiguousarray(mesh.vertices, dtype=np.float32),
            np.ascontiguousarray(mesh.triangles[::-1], dtype=np.uint32))


def tripled_case(groups, singles=0):
    """`groups` distinct triangles, each three times, and `singles` more, each once.  Without singles the first parent layer
    at degree 3 has exactly `groups` nodes: an INNER layer on the block edge (256) and one past it (257).  With ONE single
    there are 3 * groups + 1 leaves with groups + 1 distinct codes, a mean run just short of 3: the codes are shifted before
    the first parent layer -- and would not be if the count of distinct codes came out one too low.  One neighbouring pair
    lost anywhere in the leaf layer (a block edge, the tail past the histogram kernel's grid cap) gives another tree."""
    rng = np.random.default_rng(120)
    centre = rng.uniform(-50, 50, size=(groups + singles, 1, 3)).astype(np.float32)
    tri = centre + rng.normal(0, 6, size=(groups + singles, 3, 3)).astype(np.float32)
    name = 'tripled-%d' % groups + ('+%d' % singles if singles else '')
    return _own_vertices(name, np.concatenate([np.repeat(tri[:groups], 3, axis=0), tri[groups:]]))


EDGE_CASES = {}                          # name -> (generator, its arguments, the degrees compared)
for _i, _n in enumerate(SOUP_SIZES):
    EDGE_CASES['soup-%d' % _n] = (soup_case, (_n, 100 + _i), EDGE_DEGREES)
EDGE_CASES['soup-5000'] = (soup_case, (5000, 116), EDGE_DEGREES + (4, 15, 100))
for _m in IDENTICAL_COUNTS:
    EDGE_CASES['identical-%d' % _m] = (identical_case, (_m,), EDGE_DEGREES)
EDGE_CASES['planar'] = (planar_case, (), EDGE_DEGREES)
EDGE_CASES['collinear'] = (collinear_case, (), EDGE_DEGREES)
EDGE_CASES['sphere-reversed'] = (reversed_sphere_case, (), EDGE_DEGREES)
EDGE_CASES['tripled-256'] = (tripled_case, (256,), EDGE_DEGREES)
EDGE_CASES['tripled-257'] = (tripled_case, (257,), EDGE_DEGREES)
EDGE_CASES['tripled-256+1'] = (tripled_case, (256, 1), EDGE_DEGREES)
EDGE_CASES['soup-%d' % LARGE_SOUP] = (soup_case, (LARGE_SOUP, 119), (3,))
# (in the large soup the 257 leaves past 4096 x 256 hold too few of its million distinct codes to move the choice of the
#  shift: a histogram kernel without its grid-stride loop builds the same tree.  Here one lost pair is enough.)
EDGE_CASES['tripled-%d+1' % LARGE_TRIPLED] = (tripled_case, (LARGE_TRIPLED, 1), (3,))


@functools.lru_cache(maxsize=None)
def edge_case(name):
    """(vertices, triangles, world frame) of a case, made once and read-only."""
    fn, args, _ = EDGE_CASES[name]
    got_name, vertices, triangles = fn(*args)
    assert got_name == name and vertices.dtype == np.float32 and triangles.dtype == np.uint32
    vertices.setflags(write=False)
    triangles.setflags(write=False)
    from chroma_amd.bvh.grid import world_coords_for
    return vertices, triangles, world_coords_for(vertices)


def _words(nodes):
    return np.ascontiguousarray(nodes).view(np.uint32).reshape(-1, 4)


@functools.lru_cache(maxsize=None)
def numpy_tree(name, degree):
    """(node words [n][4] uint32, layer bounds) of the NumPy restatement: the comparand of the host and the device builder,
    computed once and read-only."""
    from chroma_amd.bvh.grid import _build_numpy
    vertices, triangles, wc = edge_case(name)
    nodes, bounds = _build_numpy(vertices, triangles, wc, degree)
    words, bounds = _words(nodes).copy(), np.asarray(bounds, dtype=np.int64).copy()
    words.setflags(write=False)
    bounds.setflags(write=False)
    return words, bounds


def native_tree(name, degree, ctx=None):
    """(node words, layer bounds) of the host builder, or of the device builder on `ctx`."""
    from chroma_amd import _lib
    vertices, triangles, wc = edge_case(name)
    nodes, bounds = _lib.bvh_build(vertices, triangles, wc.world_origin, wc.world_scale, degree, ctx=ctx)
    return _words(nodes), np.asarray(bounds, dtype=np.int64)


def assert_same_tree(got, want, what):
    (nodes, bounds), (ref_nodes, ref_bounds) = got, want
    assert bounds.tolist() == ref_bounds.tolist(), '%s: layer bounds %s, expected %s' % (what, bounds.tolist(), ref_bounds.tolist())
    assert nodes.dtype == np.uint32 and nodes.shape == ref_nodes.shape, what
    if not np.array_equal(nodes, ref_nodes):
        bad = np.flatnonzero((nodes != ref_nodes).any(axis=1))
        raise AssertionError('%s: %d nodes differ, first %d: %s, expected %s' % (
            what, len(bad), bad[0], nodes[bad[0]].tolist(), ref_nodes[bad[0]].tolist()))


@pytest.mark.parametrize('name', list(EDGE_CASES))
def test_native_equals_numpy_on_the_edge_cases(name):
    vertices, triangles, wc = edge_case(name)
    for degree in EDGE_CASES[name][2]:
        ref = numpy_tree(name, degree)
        assert_same_tree(native_tree(name, degree), ref, '%s, degree %d' % (name, degree))
        check_tree_invariants(BVH(wc, ref[0].view(uint4)[:, 0], ref[1][:-1].tolist()), len(triangles))


def test_the_edge_cases_reach_what_they_are_there_for():
    """Every value from the NumPy trees alone: nodes with 15 children in more than one layer, leaves lifted into inner layers
    by the collapse, and inner layers (not just leaf layers, whose sizes are the cases' own) on and one past a multiple of
    the kernels' 256-thread block."""
    def layers(name, degree):
        words, bounds = numpy_tree(name, degree)
        nchild = words[:, 3] >> CHILD_BITS
        return [nchild[lo:hi] for lo, hi in zip(bounds[:-1], bounds[1:])]

    full_layers = {name: sum(1 for l in layers(name, 3) if (l == 15).any()) for name in EDGE_CASES}
    assert max(full_layers.values()) >= 2 and full_layers['identical-3376'] >= 2, full_layers
    for name in ('identical-16', 'identical-226'):
        for degree in EDGE_DEGREES:
            inner = layers(name, degree)[:-1]
            assert len(inner) >= 2 and any((l == 0).any() for l in inner), (name, degree)
    for name in ('identical-15', 'identical-225'):                 # full nodes only: nothing to lift
        inner = layers(name, 3)[:-1]
        assert all(((l == 15) | (len(l) == 1)).all() for l in inner), name
    inner_sizes = {(name, degree): [len(l) for l in layers(name, degree)[:-1]] for name in EDGE_CASES for degree in EDGE_CASES[name][2]}
    on_edge = [k for k, sizes in inner_sizes.items() if any(s >= 256 and s % 256 == 0 for s in sizes)]
    past_edge = [k for k, sizes in inner_sizes.items() if any(s > 256 and s % 256 == 1 for s in sizes)]
    assert ('tripled-256', 3) in on_edge and ('tripled-257', 3) in past_edge, (on_edge, past_edge)
    # the cases that hang on ONE distinct code: 3 g + 1 leaves with exactly g + 1 codes, so that the codes are shifted (fewer
    # than g + 1 parents) where a count of g would have left them as they are
    from chroma_amd.bvh.grid import make_leaves_numpy
    for groups in (256, LARGE_TRIPLED):
        name = 'tripled-%d+1' % groups
        vertices, triangles, wc = edge_case(name)
        assert len(triangles) == 3 * groups + 1
        assert len(np.unique(make_leaves_numpy(vertices, triangles, wc)[1])) == groups + 1, name
        assert len(layers(name, 3)[-2]) < groups + 1, name
    assert 3 * LARGE_TRIPLED + 1 > 4096 * 256                      # (past the grid cap of the histogram kernel)
    leaf_sizes = [len(layers(name, 3)[-1]) for name in EDGE_CASES]
    assert any(s % 256 == 0 for s in leaf_sizes) and any(s % 256 == 1 and s > 1 for s in leaf_sizes)


# ---- what the builders refuse -------------------------------------------------------------------------------------------------
def _as_mesh(vertices, triangles):
    """The least make_recursive_grid_bvh asks of a mesh."""
    return types.SimpleNamespace(vertices=vertices, triangles=triangles)


def unquantisable_meshes():
    """(name, vertices, triangles) of meshes whose fixed-point frame cannot quantise: all vertices in one point (scale 0),
    one NaN vertex (origin NaN), one infinite vertex (scale inf)."""
    name, vertices, triangles = soup_case(200, 7)
    yield _own_vertices('one-point', np.full((4, 3, 3), 2.5, dtype=np.float32))
    for what, value in (('nan', np.nan), ('inf', np.inf), ('minus-inf', -np.inf)):
        v = vertices.copy()
        v[301, 1] = value
        yield what + '-vertex', v, triangles


# Degree 1 does not return where it is not refused (with distinct codes a layer of n nodes gets n one-child parents), so the
# refusal is asked for on meshes on which even an unguarded builder ends: one triangle (no parent layer at all) and 16
# identical ones (one run at every layer).
SAFE_FOR_ANY_DEGREE = ('soup-1', 'identical-16')
BAD_DEGREES = (1, 0, -3)


def test_a_target_degree_below_two_is_refused_on_the_host():
    from chroma_amd import _lib
    from chroma_amd.bvh.grid import _build_numpy
    for name in SAFE_FOR_ANY_DEGREE:
        vertices, triangles, wc = edge_case(name)
        for degree in BAD_DEGREES:
            with pytest.raises(_lib.ChromaError, match='target_degree'):
                _lib.bvh_build(vertices, triangles, wc.world_origin, wc.world_scale, degree)
            with pytest.raises(ValueError, match='target_degree'):
                _build_numpy(vertices, triangles, wc, degree)
            for backend in ('native', 'numpy'):
                with pytest.raises(ValueError, match='target_degree'):
                    make_recursive_grid_bvh(_as_mesh(vertices, triangles), target_degree=degree, backend=backend)
        assert_same_tree(native_tree(name, 2), numpy_tree(name, 2), name + ' after the refusals')


def test_a_frame_that_cannot_quantise_is_refused_on_the_host():
    from chroma_amd import _lib
    from chroma_amd.bvh.grid import world_coords_for
    good_v, good_t, good = edge_case('soup-257')
    for name, vertices, triangles in unquantisable_meshes():
        for backend in ('native', 'numpy'):
            with pytest.raises(ValueError, match='no extent or has non-finite vertices'):
                make_recursive_grid_bvh(_as_mesh(vertices, triangles), backend=backend)
        wc = world_coords_for(vertices)
        with pytest.raises(_lib.ChromaError, match='world_scale|world_origin'):
            _lib.bvh_build(vertices, triangles, wc.world_origin, wc.world_scale, 3)
    # the C entry point by itself, on a good mesh: every way the frame can be wrong
    for scale in (0.0, -good.world_scale, np.nan, np.inf, -np.inf):
        with pytest.raises(_lib.ChromaError, match='world_scale'):
            _lib.bvh_build(good_v, good_t, good.world_origin, scale, 3)
    for axis in range(3):
        for value in (np.nan, np.inf, -np.inf):
            origin = good.world_origin.copy()
            origin[axis] = value
            with pytest.raises(_lib.ChromaError, match='world_origin'):
                _lib.bvh_build(good_v, good_t, origin, good.world_scale, 3)
    assert_same_tree(native_tree('soup-257', 3), numpy_tree('soup-257', 3), 'soup-257 after the refusals')
    bvh = make_recursive_grid_bvh(_as_mesh(good_v, good_t), backend='native')
    assert np.array_equal(_words(bvh.nodes), numpy_tree('soup-257', 3)[0])


def test_a_vertex_index_outside_the_mesh_is_refused_on_the_host():
    from chroma_amd import _lib
    vertices, triangles, wc = edge_case('soup-257')
    for row, slot in ((0, 0), (len(triangles) - 1, 2)):                # the two ends of the index array
        bad = triangles.copy()
        bad[row, slot] = len(vertices)
        with pytest.raises(_lib.ChromaError, match='outside the mesh'):
            _lib.bvh_build(vertices, bad, wc.world_origin, wc.world_scale, 3)
    assert_same_tree(native_tree('soup-257', 3), numpy_tree('soup-257', 3), 'soup-257 after the refusals')
