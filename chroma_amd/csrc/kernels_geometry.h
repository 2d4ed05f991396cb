// kernels_geometry.h -- what chroma_geometry_create derives on the device from the arrays it has uploaded: the traversal copy of
// the nodes, the triangle, physics and intersection records, and the stack need of the two trees.
// One of the kernel families of libchroma_hip.so; included by geometry.hip alone, so that each kernel is compiled once.
#pragma once

// chroma_geometry_create's two derived arrays, made on the device from what has just been uploaded
__global__ void k_traversal_nodes(const uint4 *nodes, uint32_t nnodes, const uint32_t *tri_to_dev, uint32_t ntriangles, uint4 *out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nnodes) return;
    uint4 n = nodes[i];
    if ((n.w >> CHROMA_CHILD_BITS) == 0) { const uint32_t t = n.w & ~CHROMA_NCHILD_MASK; n.w = t < ntriangles ? tri_to_dev[t] : n.w; }
    out[i] = n;
}
__global__ void k_triangle_records(const float *vertices, const uint32_t *triangles, const uint32_t *codes, const uint32_t *rank,
                                   const uint32_t *dev_to_tri, uint32_t nrecords, float4 *tri)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nrecords) return;
    const uint32_t t = dev_to_tri[k];
    const uint32_t extra[3] = {codes[t], t, rank[t]};
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float *vv = vertices + 3 * (size_t)triangles[3 * (size_t)t + c];
        tri[(size_t)TRI_STRIDE * k + c] = make_float4(vv[0], vv[1], vv[2], __uint_as_float(extra[c]));
    }
}
// the 32-byte physics records (TriPhys, device_common.h), one per 48-byte record and in the same order: the normal by
// fill_state's expression and the leaf box by the reference's rule, from the record's vertices, in k_physics's arithmetic
__global__ void k_triangle_phys(GeoView g, uint32_t nrecords, uint4 *out)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nrecords) return;
    const float4 *t = g.tri + (size_t)TRI_STRIDE * k;
    const float4 a = t[0], b = t[1], c = t[2];
    const v3 v0 = mk3(a.x, a.y, a.z), v1 = mk3(b.x, b.y, b.z), v2 = mk3(c.x, c.y, c.z);
    const v3 n = triangle_normal(v0, v1, v2);
    uint32_t bx, by, bz;
    leaf_words(g, v0, v1, v2, bx, by, bz);
    out[2 * (size_t)k] = make_uint4(__float_as_uint(n.x), __float_as_uint(n.y), __float_as_uint(n.z), __float_as_uint(a.w));
    out[2 * (size_t)k + 1] = make_uint4(__float_as_uint(b.w), bx, by, bz);
}
// the 48-byte intersection records (GeoView::tri_isect, device_common.h), one per triangle record and in the same order:
// the edges by intersect_triangle's expressions (v1 - v0, v2 - v0 in float), laid out for intersect_triangle_edges
__global__ void k_triangle_isect(GeoView g, uint32_t nrecords, float4 *out)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nrecords) return;
    const float4 *t = g.tri + (size_t)TRI_STRIDE * k;
    const float4 a = t[0], b = t[1], c = t[2];
    const v3 v0 = mk3(a.x, a.y, a.z), e1 = mk3(b.x, b.y, b.z) - v0, e2 = mk3(c.x, c.y, c.z) - v0;
    out[3 * (size_t)k] = make_float4(e1.x, e2.x, e1.y, e2.y);
    out[3 * (size_t)k + 1] = make_float4(e1.z, e2.z, v0.x, v0.y);
    out[3 * (size_t)k + 2] = make_float4(v0.z, c.w, 0.0f, 0.0f);
}
// Worst-case number of simultaneously live stack entries of the depth-first walk in
// intersect_mesh for this tree (every box test succeeding).  Children always have larger
// indices than their parent (layers are stored root first), so one backward sweep suffices.
// Most entries a walk's stack can hold at once, for the two trees of a geometry, from the arrays AS UPLOADED.
// need(node) = max over its inner children c, in push order, of (inner children before c) + need(c) [reference walk, mesh.h:68-110],
// need(node) = inner children - 1 + max need(child) [nearest-first wide walk].  Children follow their parents in both arrays, so
// the values are the least fixed point of these rules: every pass over the array only raises entries, and after (depth of the
// tree) passes nothing changes -- ~30 passes of a few milliseconds instead of a second-long backward sweep on one host core.
__global__ void k_stack_need_ref(const uint4 *nodes, uint32_t nnodes, uint32_t *need, uint32_t *changed)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nnodes) return;
    const uint32_t w = nodes[i].w, nchild = w >> CHROMA_CHILD_BITS, first = w & ~CHROMA_NCHILD_MASK;
    if (nchild == 0) return;
    uint32_t best = 0;
    if ((uint64_t)first + nchild > nnodes || first <= i) best = 0xFFFFu;
    else {
        uint32_t rank = 0;
        for (uint32_t j = 0; j < nchild; j++)
            if ((nodes[first + j].w >> CHROMA_CHILD_BITS) != 0) { best = max(best, rank + need[first + j]); rank++; }
        best = min(max(best, rank), 0xFFFFu);
    }
    if (best != need[i]) { need[i] = best; *changed = 1u; }
}
__global__ void k_stack_need_wide(const uint4 *wnodes, uint32_t nwide, uint32_t *need, uint32_t *changed)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nwide) return;
    uint32_t inner = 0, below = 0;
    for (int j = 0; j < 8; j++) {
        const uint32_t w = wnodes[8 * (size_t)i + j].w;
        if (w == 0xFFFFFFFFu || (w & 0x80000000u)) continue;
        inner++;
        if (w < nwide && w > i) below = max(below, need[w]);
    }
    const uint32_t v = min(0xFFFFu, inner ? inner - 1u + below : 0u);
    if (v != need[i]) { need[i] = v; *changed = 1u; }
}
