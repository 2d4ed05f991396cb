// ref_pdf_driver.cc -- TEST INFRASTRUCTURE.  A HOST driver around the reference's OWN PDF kernels, compiled by g++
// from where they lie (found through -I, see oracle/Makefile; nothing is copied): chroma/cuda/pdf.cu (bin_hits :9-32,
// accumulate_bincount :34-96, accumulate_nearest_neighbor :98-150, accumulate_moments :223-265,
// accumulate_kernel_eval :271-368) with sorting.h (piksrt).  The CUDA words those sources use come from the stand-ins
// of oracle/ref_shim (the project's own text).
//
// One build, against the host libm (libchroma_ref_pdf.so): the device kernels of chroma_amd/csrc/kernels_pdf.h call
// expf / erff, not the contract of include/chroma_math.h.
//
// One host thread runs every thread of a kernel in order, thread 0 first (see ref_shim/cuda_host_shim.h).  Each entry
// point below runs ONE reference kernel over all its threads; what the reference's Python layer does around a launch
// (chroma/gpu/pdf.py: the work queues filled with 1, one launch per DAQ copy) is done here and said where.
//
// The reference is defined on less than the project's kernels are: charges in [0, 2^32), no time
// whose bin index rounds up to tbins, no NaN, and at most 1000 distances per hit channel and call.  The callers keep
// to that domain; the one limit that would write out of bounds HERE (distance_table[1000]) is refused below.
#include <vector>

#include "cuda_host_shim.h"
#include "curand_kernel.h"

#include "pdf.cu"

namespace {

const int kThreadsPerBlock = 64;          // chroma/gpu/pdf.py: nthreads_per_block=64

template <class Body> void launch(uint32_t nthreads, Body body)
{
    blockDim.x = kThreadsPerBlock; blockDim.y = blockDim.z = 1;
    const uint32_t nblocks = nthreads / kThreadsPerBlock + 1;          // the reference's grid: one block too many at a multiple
    gridDim.x = nblocks; gridDim.y = gridDim.z = 1;
    for (uint32_t b = 0; b < nblocks; b++)
        for (uint32_t t = 0; t < (uint32_t)kThreadsPerBlock; t++) {
            blockIdx.x = b; threadIdx.x = t;
            body();
        }
}

}  // namespace

extern "C" {

const char *ref_pdf_variant(void) { return "libm"; }

// The size of the reference's per-thread distance_table (pdf.cu:118).
int32_t ref_pdf_table_size(void) { return 1000; }

// bin_hits once per copy, in copy order, at copy * stride.  `pdf`: the caller's [nchannels + guard rows][tbins][qbins].
int32_t ref_pdf_bin_hits(int32_t nchannels, int32_t ndaq, uint32_t stride, float *channel_q, float *channel_t, uint32_t *hitcount,
                         int32_t tbins, float tmin, float tmax, int32_t qbins, float qmin, float qmax, uint32_t *pdf)
{
    if (nchannels < 0 || ndaq < 1 || stride < (uint32_t)nchannels || tbins < 1 || qbins < 1) return -1;
    for (int32_t i = 0; i < ndaq; i++) {
        float *q = channel_q + (size_t)i * stride, *t = channel_t + (size_t)i * stride;
        launch((uint32_t)nchannels, [&] { bin_hits(nchannels, q, t, hitcount, tbins, tmin, tmax, qbins, qmin, qmax, pdf); });
    }
    return 0;
}

// accumulate_bincount, then accumulate_nearest_neighbor, as accumulate_pdf_eval of chroma/gpu/pdf.py launches them:
// work queues of nhit * (ndaq + 1) words filled with 1 before the call.  `mc_time`: ndaq copies PACKED at stride
// nchannels (accumulate_bincount reads nchannels * i + channel).  `channel_to_hit`: max(0, cumsum(event_hit) - 1);
// `hit_to_channel`: the hit channels ascending; `nearest`: [nhit][k].  An event with no hit channel still gets one
// queue: every unhit channel reads work_queue[0] of queue 0.  Refused without a call (-2): k + ndaq > 1000, the old
// entries plus one call's queue that distance_table[1000] has to hold.
int32_t ref_pdf_eval_accumulate(int32_t nchannels, int32_t ndaq, uint32_t *event_hit, float *event_time, float *mc_time,
                                uint32_t *hitcount, uint32_t *bincount, float min_twidth, float tmin, float tmax, int32_t k,
                                int32_t nhit, uint32_t *channel_to_hit, uint32_t *hit_to_channel, float *nearest)
{
    if (nchannels < 0 || ndaq < 1 || k < 1 || nhit < 0 || nhit > nchannels) return -1;
    if ((int64_t)k + ndaq > ref_pdf_table_size()) return -2;
    std::vector<uint32_t> work_queues((size_t)(nhit > 0 ? nhit : 1) * ((size_t)ndaq + 1), 1u);
    launch((uint32_t)nchannels, [&] {
        accumulate_bincount(nchannels, ndaq, event_hit, event_time, mc_time, hitcount, bincount, min_twidth, tmin, tmax, k,
                            channel_to_hit, work_queues.data());
    });
    launch((uint32_t)nhit, [&] {
        accumulate_nearest_neighbor(nhit, ndaq, hit_to_channel, work_queues.data(), event_time, mc_time, nearest, k);
    });
    return 0;
}

// accumulate_moments once per copy, in copy order, at copy * stride.
int32_t ref_pdf_moments(int32_t time_only, int32_t nchannels, int32_t ndaq, uint32_t stride, float *mc_time, float *mc_charge,
                        float tmin, float tmax, float qmin, float qmax, uint32_t *mom0, float *t_mom1, float *t_mom2,
                        float *q_mom1, float *q_mom2)
{
    if (nchannels < 0 || ndaq < 1 || stride < (uint32_t)nchannels) return -1;
    for (int32_t i = 0; i < ndaq; i++) {
        float *t = mc_time + (size_t)i * stride, *q = mc_charge + (size_t)i * stride;
        launch((uint32_t)nchannels, [&] {
            accumulate_moments(time_only, nchannels, t, q, tmin, tmax, qmin, qmax, mom0, t_mom1, t_mom2, q_mom1, q_mom2);
        });
    }
    return 0;
}

// accumulate_kernel_eval once per copy, in copy order, at copy * stride.
int32_t ref_pdf_kernel_eval(int32_t time_only, int32_t nchannels, int32_t ndaq, uint32_t stride, uint32_t *event_hit,
                            float *event_time, float *event_charge, float *mc_time, float *mc_charge, float tmin, float tmax,
                            float qmin, float qmax, float *inv_time_bandwidths, float *inv_charge_bandwidths, uint32_t *hitcount,
                            float *time_pdf_values, float *charge_pdf_values)
{
    if (nchannels < 0 || ndaq < 1 || stride < (uint32_t)nchannels) return -1;
    for (int32_t i = 0; i < ndaq; i++) {
        float *t = mc_time + (size_t)i * stride, *q = mc_charge + (size_t)i * stride;
        launch((uint32_t)nchannels, [&] {
            accumulate_kernel_eval(time_only, nchannels, event_hit, event_time, event_charge, t, q, tmin, tmax, qmin, qmax,
                                   inv_time_bandwidths, inv_charge_bandwidths, hitcount, time_pdf_values, charge_pdf_values);
        });
    }
    return 0;
}

}  // extern "C"
