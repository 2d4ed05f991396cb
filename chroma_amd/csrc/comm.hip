// comm.hip -- the hit reduction across the GPUs of a node: RCCL found with dlopen, chroma_comm_*, chroma_allreduce_*.
#include <string.h>
#include <dlfcn.h>

#include "chroma_internal.h"

// ---- the hit reduction across GPUs ----------------------------------------------------
// Photons never interact and every GPU holds the whole geometry, so a batch sharded over the GPUs of a
// node needs exactly one exchange: its per-channel arrays.  That exchange is RCCL on the library's own
// stream, on the device arrays the hit kernels filled -- nothing is staged through the host.  RCCL is
// found with dlopen when the first communicator call is made (a process that already holds an RCCL, e.g.
// torch's, gets that one through the shared-object name), so single-GPU users never load it.
struct RcclApi {
    void *handle = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
};
static RcclApi g_rccl;

static int rccl_load()
{
    if (g_rccl.handle) return CHROMA_OK;
    void *h = nullptr;
    for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
        h = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
        if (h) break;
    }
    if (!h) return set_error(CHROMA_ERR_INVALID, "RCCL not found (dlopen librccl.so.1): %s", dlerror());
#define SYM(field, name) \
    do { *(void **)(&g_rccl.field) = dlsym(h, name); \
         if (!g_rccl.field) { dlclose(h); return set_error(CHROMA_ERR_INVALID, "RCCL: symbol %s missing", name); } } while (0)
    SYM(GetUniqueId, "ncclGetUniqueId"); SYM(CommInitRank, "ncclCommInitRank"); SYM(CommDestroy, "ncclCommDestroy");
    SYM(AllReduce, "ncclAllReduce"); SYM(AllGather, "ncclAllGather"); SYM(GroupStart, "ncclGroupStart");
    SYM(GroupEnd, "ncclGroupEnd"); SYM(GetErrorString, "ncclGetErrorString");
#undef SYM
    g_rccl.handle = h;
    return CHROMA_OK;
}
#define RCCL_TRY(expr)                                                                             \
    do {                                                                                           \
        ncclResult_t r_ = (expr);                                                                  \
        if (r_ != ncclSuccess)                                                                     \
            return set_error(CHROMA_ERR_INVALID, "%s failed: %s", #expr, g_rccl.GetErrorString(r_)); \
    } while (0)

extern "C" {

#include "kernels_comm.h"          // (in here: k_or_gathered keeps its unmangled name)

int chroma_comm_unique_id(uint8_t id[CHROMA_COMM_ID_BYTES])
{
    if (!id) return set_error(CHROMA_ERR_INVALID, "null id");
    static_assert(CHROMA_COMM_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "id size");
    int rc = rccl_load(); if (rc) return rc;
    ncclUniqueId u;
    RCCL_TRY(g_rccl.GetUniqueId(&u));
    memcpy(id, u.internal, NCCL_UNIQUE_ID_BYTES);
    return CHROMA_OK;
}

int chroma_comm_init(chroma_ctx *ctx, int32_t nranks, int32_t rank, const uint8_t id[CHROMA_COMM_ID_BYTES])
{
    if (!ctx || !id || nranks < 1 || rank < 0 || rank >= nranks) return set_error(CHROMA_ERR_INVALID, "bad argument");
    if (ctx->comm) return set_error(CHROMA_ERR_INVALID, "this context already has a communicator");
    int rc = rccl_load(); if (rc) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    ncclUniqueId u;
    memcpy(u.internal, id, NCCL_UNIQUE_ID_BYTES);
    RCCL_TRY(g_rccl.CommInitRank(&ctx->comm, nranks, u, rank));
    ctx->comm_nranks = nranks;
    ctx->comm_rank = rank;
    return CHROMA_OK;
}

int chroma_comm_destroy(chroma_ctx *ctx)
{
    if (!ctx) return set_error(CHROMA_ERR_INVALID, "null ctx");
    if (ctx->comm) {
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        RCCL_TRY(g_rccl.CommDestroy(ctx->comm));
        ctx->comm = nullptr;
        ctx->comm_nranks = 1;
        ctx->comm_rank = 0;
    }
    if (ctx->gather_buf) { hipFree(ctx->gather_buf); ctx->gather_buf = nullptr; ctx->gather_capacity = 0; }
    return CHROMA_OK;
}

// hit_count: sum; earliest-time bit patterns: min (non-negative times order like their bits,
// chroma/cuda/daq.cu:5-20).  In place, on the library's stream; without a communicator the arrays
// already are the whole job's.
int chroma_allreduce_hits(chroma_ctx *ctx, uint32_t *d_hit_count, uint32_t *d_earliest_time_bits, uint32_t nchannels)
{
    if (!ctx || !d_hit_count) return set_error(CHROMA_ERR_INVALID, "bad argument");
    if (!ctx->comm || nchannels == 0) return CHROMA_OK;
    // (the first error is kept and the group is ALWAYS closed: an early return between GroupStart and GroupEnd would
    //  leave the group open for every later RCCL call of the process -- torch's included, the library is shared)
    RCCL_TRY(g_rccl.GroupStart());
    ncclResult_t first = g_rccl.AllReduce(d_hit_count, d_hit_count, nchannels, ncclUint32, ncclSum, ctx->comm, ctx->stream);
    if (first == ncclSuccess && d_earliest_time_bits)
        first = g_rccl.AllReduce(d_earliest_time_bits, d_earliest_time_bits, nchannels, ncclUint32, ncclMin, ctx->comm, ctx->stream);
    const ncclResult_t end = g_rccl.GroupEnd();
    if (first == ncclSuccess) first = end;
    if (first != ncclSuccess) return set_error(CHROMA_ERR_INVALID, "chroma_allreduce_hits: %s", g_rccl.GetErrorString(first));
    return CHROMA_OK;
}

// The three integer arrays a DAQ acquisition accumulates (chroma/cuda/daq.cu:73-75) over sharded photons:
// earliest time bits (min), integer charge (sum), channel histories (bitwise OR -- not an RCCL reduction:
// all-gather, then OR locally).
int chroma_allreduce_daq(chroma_ctx *ctx, uint32_t *d_earliest_time_int, uint32_t *d_channel_q_int,
                         uint32_t *d_channel_histories, uint32_t nchannels)
{
    if (!ctx || !d_earliest_time_int || !d_channel_q_int || !d_channel_histories) return set_error(CHROMA_ERR_INVALID, "bad argument");
    if (!ctx->comm || nchannels == 0) return CHROMA_OK;
    const size_t need = (size_t)ctx->comm_nranks * nchannels;
    if (ctx->gather_capacity < need) {
        HIP_TRY(hipSetDevice(ctx->device));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        if (ctx->gather_buf) hipFree(ctx->gather_buf);
        ctx->gather_buf = nullptr; ctx->gather_capacity = 0;
        HIP_TRY(hipMalloc((void **)&ctx->gather_buf, need * sizeof(uint32_t)));
        ctx->gather_capacity = need;
    }
    RCCL_TRY(g_rccl.GroupStart());
    ncclResult_t first = g_rccl.AllReduce(d_earliest_time_int, d_earliest_time_int, nchannels, ncclUint32, ncclMin, ctx->comm, ctx->stream);
    if (first == ncclSuccess)
        first = g_rccl.AllReduce(d_channel_q_int, d_channel_q_int, nchannels, ncclUint32, ncclSum, ctx->comm, ctx->stream);
    if (first == ncclSuccess)
        first = g_rccl.AllGather(d_channel_histories, ctx->gather_buf, nchannels, ncclUint32, ctx->comm, ctx->stream);
    const ncclResult_t end = g_rccl.GroupEnd();          // (always: see chroma_allreduce_hits)
    if (first == ncclSuccess) first = end;
    if (first != ncclSuccess) return set_error(CHROMA_ERR_INVALID, "chroma_allreduce_daq: %s", g_rccl.GetErrorString(first));
    hipLaunchKernelGGL(k_or_gathered, dim3((nchannels + 255) / 256), dim3(256), 0, ctx->stream, d_channel_histories,
                       ctx->gather_buf, nchannels, ctx->comm_nranks);
    HIP_TRY(hipGetLastError());
    return CHROMA_OK;
}

}  // extern "C"
