"""k_raycast_quad's quad reductions and its stack at the edge of the LDS part, seen through the walk.

The reductions (quad_or_u32, quad_min_u32, quad_max_u32 of kernel_raycast_quad.h) compile to DPP operations on the value
itself; what they must give -- the same word in all four lanes of a ray -- shows in the walk's answers: the decision word
steers the ring and the stack, the minimum picks the next child and the nearest hit, and the rank minimum and the triangle
maximum decide ties.  So small bundles of chroma_distance_to_mesh under the default walk are held against
oracle.distance_to_mesh bit for bit, with rays through shared vertices and edge midpoints among them that meet two
triangles at the same distance bits.

The stack: rays of demo.tiny() whose stack reaches 3, 4, 5 entries and the deepest any candidate reached, cast with the
library built with 4 entries in LDS (the geometry and the variant tests/test_gpu_spill.py uses).  tests/golden/
quad_stack_edge.npz holds the rays, the depth each reaches when it is cast alone, and the entries the parent of this change
pushed through the spill area, per ray cast alone and per depth with the rays of a depth cast as one bundle, with that bundle's
node and triangle-test counts (recorded once
with a counting build of the parent that also reported the depth).  A ray's walk depends on the rays that share its wave --
a triangle round runs when any of them has eight postponed, and an earlier hit prunes more -- so a count is only the same
from run to run for a bundle of up to 16 rays: one chunk, one wave.  The bundles of one depth are such bundles.
"""
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from test_gpu_parity import _aimed_photons
from test_gpu_ray_bundle import GUARD, SENTINEL, UNWRITTEN, Rays, inside_rays, oracle_cast, same

pytestmark = pytest.mark.gpu

SIZES = (1, 15, 16, 17, 63, 64, 65, 257)
AIMED = 10
VARIANT = os.path.join(ROOT, 'build_variants', 'libchroma_hip_stack4.so')


def distance_to_mesh(ctx, gg, rays, n, counting=False):
    """One chroma_distance_to_mesh call over the first n rays under the default walk, on guarded and poisoned outputs.
    Returns ((distance bits, triangles), stats or None)."""
    from chroma_amd import _lib
    from chroma_amd.gpu.tools import GPUArray
    dist = GPUArray(n + GUARD, np.uint32, ctx).fill(np.uint32(SENTINEL))
    tri = GPUArray(n + GUARD, np.int32, ctx).fill(np.int32(UNWRITTEN))
    stats = None
    try:
        ctx.set_counting(counting)
        if counting:
            ctx.read_stats()                                   # (reading starts the counters again at zero)
        _lib.check(ctx._lib.chroma_distance_to_mesh(ctx.handle, gg.handle, n, rays.d_o.ptr, rays.d_d.ptr, dist.ptr, tri.ptr))
        if counting:
            stats = ctx.read_stats()
    finally:
        ctx.set_counting(False)
    gd, gt = dist.get(), tri.get()
    assert (gd[n:] == SENTINEL).all() and (gt[n:] == UNWRITTEN).all(), '%d rays: written past n' % n
    return (gd[:n], gt[:n]), stats


@pytest.fixture(scope='module')
def tie_rays(oracle_mod, tiny_geometry, tiny_packed):
    """Rays from the centre through shared vertices and edge midpoints which, by the oracle, meet two triangles at the same
    distance bits (with the winner excluded the ray finds another triangle exactly as far): the rank decides them."""
    ph = _aimed_photons(tiny_geometry, (0.0, 0.0, 0.0), 1)
    ntri = min(len(tiny_geometry.mesh.triangles), 6000)
    # (_aimed_photons: 3 ntri vertex targets, then 3 ntri edge midpoints, then ntri centroids)
    pick = np.concatenate([np.arange(0, 3 * ntri, 15), np.arange(3 * ntri, 6 * ntri, 15)])
    o, d = ph.pos[pick].astype(np.float32), ph.dir[pick].astype(np.float32)
    plain = oracle_cast(oracle_mod, tiny_packed, o, d)
    excluded = oracle_cast(oracle_mod, tiny_packed, o, d, plain[1])
    tie = (plain[1] >= 0) & (excluded[1] >= 0) & (excluded[1] != plain[1]) & (excluded[0] == plain[0])
    print('%d of %d aimed rays tie' % (tie.sum(), len(pick)))
    assert tie.sum() >= 8 * AIMED
    return o[tie], d[tie]


def bundle(tie_rays, k, n):
    """Bundle k: n rays from inside the detector, min(n, 10) of them rays that tie (ten other ones per bundle), spread evenly
    over the bundle and so over the quads of its waves."""
    o, d = inside_rays(np.random.default_rng(1000 + n), n)
    slots = np.unique(np.linspace(0, n - 1, min(n, AIMED)).astype(int))
    take = (AIMED * k + np.arange(len(slots))) % len(tie_rays[0])
    o[slots], d[slots] = tie_rays[0][take], tie_rays[1][take]
    return o, d, slots


@pytest.fixture(scope='module')
def product(tiny_geometry):
    from chroma_amd import gpu as g
    ctx = g.create_cuda_context(0)
    yield ctx, g.GPUDetector(tiny_geometry)
    ctx.pop()


@pytest.mark.parametrize('k', range(len(SIZES)))
def test_small_bundles_with_ties_are_the_oracles_rows(product, oracle_mod, tiny_packed, tie_rays, k):
    ctx, gg = product
    n = SIZES[k]
    o, d, slots = bundle(tie_rays, k, n)
    want = oracle_cast(oracle_mod, tiny_packed, o, d)
    assert (want[1][slots] >= 0).all()
    for counting in (False, True):
        got, stats = distance_to_mesh(ctx, gg, Rays(ctx, o, d), n, counting)
        same(got, want, '%d rays%s' % (n, ', counting' if counting else ''))
        if counting:
            assert stats['stack_overflows'] == 0 and stats['stack_spills'] == 0, stats


# ---- the stack at the edge of its LDS part -----------------------------------------------------------------------------
@pytest.fixture(scope='module')
def edge():
    return np.load(os.path.join(GOLDEN, 'quad_stack_edge.npz'))


@pytest.fixture(scope='module')
def stack4(tiny_geometry):
    from chroma_amd import gpu as g
    if not os.path.exists(VARIANT):
        pytest.fail('%s is not built: run `make -C chroma_amd/csrc variants` (build() does)' % VARIANT)
    ctx = g.create_cuda_context(0, library=VARIANT)
    yield ctx, g.GPUDetector(tiny_geometry)
    ctx.pop()


def test_the_recorded_rays_sit_on_the_edge(edge):
    lds, deepest, depth, spills = int(edge['lds_entries']), int(edge['deepest']), edge['depth'], edge['parent_spills']
    assert lds == 4 and deepest > lds + 1
    for want in (lds - 1, lds, lds + 1, deepest):
        assert (depth == want).sum() >= (1 if want == deepest else 8), want
    assert (spills[depth <= lds] == 0).all() and (spills[depth > lds] >= depth[depth > lds] - lds).all()


@pytest.mark.parametrize('which', ['below', 'full', 'one over', 'deepest', 'all'])
def test_stack_depths_around_the_lds_part(stack4, oracle_mod, tiny_packed, edge, which):
    """Depth QUAD_STACK - 1, QUAD_STACK, QUAD_STACK + 1, the deepest, and all of them in one bundle: the oracle's rows, no
    overflow, and as many entries through the spill area, node entries and triangle tests as the parent's for the same bundle."""
    ctx, gg = stack4
    lds, deepest, depth = int(edge['lds_entries']), int(edge['deepest']), edge['depth']
    pick = {'below': depth == lds - 1, 'full': depth == lds, 'one over': depth == lds + 1, 'deepest': depth == deepest,
            'all': np.ones(len(depth), bool)}[which]
    o, d = edge['origins'][pick], edge['directions'][pick]
    want = oracle_cast(oracle_mod, tiny_packed, o, d)
    got, stats = distance_to_mesh(ctx, gg, Rays(ctx, o, d), len(o), counting=True)
    same(got, want, 'stack depth: %s' % which)
    print('%s: %d rays, stack_spills %d' % (which, len(o), stats['stack_spills']))
    assert stats['stack_overflows'] == 0
    if which == 'all':               # (several waves: which rays share one is not the same in every run)
        assert stats['stack_spills'] >= edge['group_parent_spills'].max()
    else:
        assert pick.sum() <= 16
        want_depth = {'below': lds - 1, 'full': lds, 'one over': lds + 1, 'deepest': deepest}[which]
        k = list(edge['group_depth']).index(want_depth)
        assert stats['stack_spills'] == edge['group_parent_spills'][k]
        # the same walk: node entries tested and triangle tests of the bundle, as the parent counted them
        print('nodes %d, triangle tests %d' % (stats['nodes_visited'], stats['triangles_tested']))
        assert stats['nodes_visited'] == edge['group_parent_nodes'][k] and stats['triangles_tested'] == edge['group_parent_tests'][k]
    same(distance_to_mesh(ctx, gg, Rays(ctx, o, d), len(o))[0], want, 'stack depth: %s, not counting' % which)
