// kernels_pdf.h -- per-channel PDFs and likelihood terms over DAQ output (chroma/cuda/pdf.cu semantics).
//
// Every kernel reads the GPUChannels layout: `ndaq` copies of `nchannels` entries, copy i at [i * stride, i * stride +
// nchannels).  A channel time >= 1e8 means "not hit in the MC" (the DAQ writes 1e9).  The copies of one channel are
// taken in copy order inside one thread (or one wave), so K copies in one call give the same bits as K calls of one copy.
// Every window test is written in the positive form (t >= tmin && t <= tmax): a NaN time or charge is "not hit" in all
// five kernels, where the reference's negative forms (t < tmin || t > tmax) let it through.

// ---- bin_hits (pdf.cu:9-32) --------------------------------------------------------------------------
// One thread per channel.  Charge truncated to an unsigned integer (negative or NaN -> 0, saturating at 2^32 - 1).
// Bin indices are clamped to [0, bins - 1]: (t - tmin) / (tmax - tmin) * tbins can round up to tbins for t just below tmax.
__global__ void __launch_bounds__(256) k_pdf_bin_hits(uint32_t nchannels, int ndaq, uint32_t stride, const float *__restrict__ channel_q,
                                                      const float *__restrict__ channel_t, uint32_t *__restrict__ hitcount,
                                                      int tbins, float tmin, float tmax, int qbins, float qmin, float qmax,
                                                      uint32_t *__restrict__ pdf)
{
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nchannels) return;
    uint32_t *hist = pdf + (size_t)c * (size_t)tbins * (size_t)qbins;
    uint32_t count = 0;
    for (int i = 0; i < ndaq; i++) {
        const size_t at = (size_t)i * stride + c;
        const float t = channel_t[at], qf = channel_q[at];
        const uint32_t q = !(qf > 0.0f) ? 0u : (qf >= 4294967296.0f ? 0xFFFFFFFFu : (uint32_t)qf);
        const float qq = (float)q;
        if (!(t < 1e8f && t >= tmin && t < tmax && qq >= qmin && qq < qmax)) continue;
        count++;
        int tbin = (int)((t - tmin) / (tmax - tmin) * (float)tbins);
        int qbin = (int)((qq - qmin) / (qmax - qmin) * (float)qbins);
        tbin = min(max(tbin, 0), tbins - 1);
        qbin = min(max(qbin, 0), qbins - 1);
        hist[tbin * qbins + qbin] += 1;          // row major (channel, tbin, qbin); this thread owns the channel's row
    }
    if (count) hitcount[c] += count;
}

// ---- accumulate_bincount + accumulate_nearest_neighbor (pdf.cu:34-219), unhit channels ---------------------
// Channels the event did not hit only count the MC hits inside [tmin, tmax] (inclusive at tmax, unlike bin_hits).
__global__ void __launch_bounds__(256) k_pdf_eval_hitcount(uint32_t nchannels, int ndaq, uint32_t stride,
                                                           const uint32_t *__restrict__ event_hit,
                                                           const float *__restrict__ mc_time, float tmin, float tmax,
                                                           uint32_t *__restrict__ hitcount)
{
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nchannels || event_hit[c]) return;
    uint32_t count = 0;
    for (int i = 0; i < ndaq; i++) {
        const float mc = mc_time[(size_t)i * stride + c];
        if (!(mc < 1e8f && mc >= tmin && mc <= tmax)) continue;
        count++;
    }
    if (count) hitcount[c] += count;
}

// Hit channels: one wave64 per channel in hit_channels[], 64 copies per round.
//  - valid copy: MC time < 1e8 and inside [tmin, tmax] (a NaN is neither) -> hitcount += 1
//  - in the minimum bin: |mc - event_time| < min_twidth / 2 -> bincount += 1
//  - candidate: valid and the running bincount (after this copy) < min_bin_content; the running count of lane L is the
//    count before the round plus the in-bin lanes <= L (ballot + mbcnt).  A NaN distance (NaN event time) is never a
//    candidate: the sorting network's fminf / fmaxf would drop it and duplicate its partner
//  - nearest[h * k .. h * k + k) holds the k = min_bin_content smallest candidate distances so far, ascending, padded
//    with 1e9.  A round's candidates are sorted across the wave (bitonic network on lane shuffles) and merged into it
//    by rank: old entry i goes to i + #(new < it), new entry j to j + #(old <= it); ranks >= k are dropped.  In place:
//    one wave owns the list and its loads and stores to it are ordered as written.
#define PDF_EVAL_WAVES 4
__device__ __forceinline__ uint32_t pdf_lane_prefix(uint64_t mask)          // set bits of `mask` below this lane
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

__global__ void __launch_bounds__(64 * PDF_EVAL_WAVES) k_pdf_eval_accumulate(
    uint32_t nchannels, int ndaq, uint32_t stride, uint32_t nhit, const uint32_t *__restrict__ hit_channels,
    const uint32_t *__restrict__ event_hit, const float *__restrict__ event_time, const float *__restrict__ mc_time,
    float half_twidth, float tmin, float tmax, int k, uint32_t *__restrict__ hitcount, uint32_t *__restrict__ bincount,
    float *nearest)
{
    const uint32_t h = blockIdx.x * PDF_EVAL_WAVES + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (h >= nhit) return;                                  // wave-uniform
    const uint32_t c = hit_channels[h];
    if (c >= nchannels || !event_hit[c]) return;
    const float et = event_time[c];
    float *list = nearest + (size_t)h * (size_t)k;
    uint32_t nvalid = 0, nbin = bincount[c];
    for (int base = 0; base < ndaq; base += 64) {
        const int i = base + lane;
        float mc = 1e9f;
        if (i < ndaq) mc = mc_time[(size_t)i * stride + c];
        const bool valid = mc < 1e8f && mc >= tmin && mc <= tmax;
        const float d = fabsf(mc - et);
        const bool inbin = valid && d < half_twidth;
        const uint64_t binmask = __ballot(inbin);
        const uint32_t running = nbin + pdf_lane_prefix(binmask) + (inbin ? 1u : 0u);
        const bool cand = valid && d == d && running < (uint32_t)k;
        const uint64_t candmask = __ballot(cand);
        nvalid += (uint32_t)__popcll(__ballot(valid));
        nbin += (uint32_t)__popcll(binmask);
        if (candmask == 0) continue;                        // wave-uniform

        // sort the candidates ascending across the wave; the other lanes carry +inf to the end
        float v = cand ? d : __builtin_inff();
#pragma unroll
        for (int size = 2; size <= 64; size <<= 1) {
#pragma unroll
            for (int stride_ = size >> 1; stride_ > 0; stride_ >>= 1) {
                const float o = __shfl_xor(v, stride_);
                const bool take_min = ((lane & stride_) == 0) == ((lane & size) == 0);
                v = take_min ? fminf(v, o) : fmaxf(v, o);
            }
        }
        const int ncand = __popcll(candmask);

        // ranks of the new entries among the old (count of old <= new): binary search of the old list, before any write
        int new_pos = k;
        if (lane < ncand) {
            int lo = 0;
            for (int step = 1024; step > 0; step >>= 1) {
                const int probe = lo + step - 1;
                if (probe < k && list[probe] <= v) lo += step;
            }
            new_pos = lane + lo;
        }
        // the old entries move up by their count of new < old: taken 64 at a time from the top, so a move only
        // overwrites entries of its own group (read by the same load) or of groups already moved
        for (int s = (k - 1) >> 6; s >= 0; s--) {
            const int at = s * 64 + lane;
            const float old = at < k ? list[at] : __builtin_inff();
            int lo = 0;
#pragma unroll
            for (int step = 64; step > 0; step >>= 1) {
                const int probe = lo + step - 1;
                const float b = __shfl(v, probe & 63);
                if (probe < ncand && b < old) lo += step;
            }
            __asm__ __volatile__("" ::: "memory");
            if (at < k && at + lo < k) list[at + lo] = old;
        }
        if (new_pos < k) list[new_pos] = v;         // below or among the moved entries, at the slots they left
    }
    if (lane == 0) {
        hitcount[c] += nvalid;
        bincount[c] = nbin;
    }
}

// ---- accumulate_moments (pdf.cu:223-265) -------------------------------------------------------------
__global__ void __launch_bounds__(256) k_pdf_moments(int time_only, uint32_t nchannels, int ndaq, uint32_t stride,
                                                     const float *__restrict__ mc_time, const float *__restrict__ mc_charge,
                                                     float tmin, float tmax, float qmin, float qmax,
                                                     uint32_t *__restrict__ mom0, float *__restrict__ t_mom1,
                                                     float *__restrict__ t_mom2, float *__restrict__ q_mom1,
                                                     float *__restrict__ q_mom2)
{
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nchannels) return;
    uint32_t m0 = mom0[c];
    float t1 = t_mom1[c], t2 = t_mom2[c];
    float q1 = 0.0f, q2 = 0.0f;
    if (!time_only) { q1 = q_mom1[c]; q2 = q_mom2[c]; }
    for (int i = 0; i < ndaq; i++) {
        const size_t at = (size_t)i * stride + c;
        const float t = mc_time[at];
        if (!(t >= tmin && t <= tmax)) continue;
        if (time_only) {
            m0 += 1;
            t1 += t;
            t2 += t * t;
        } else {
            const float q = mc_charge[at];
            if (!(q >= qmin && q <= qmax)) continue;
            m0 += 1;
            t1 += t;
            t2 += t * t;
            q1 += q;
            q2 += q * q;
        }
    }
    mom0[c] = m0;
    t_mom1[c] = t1;
    t_mom2[c] = t2;
    if (!time_only) { q_mom1[c] = q1; q_mom2[c] = q2; }
}

// ---- accumulate_kernel_eval (pdf.cu:267-368) ---------------------------------------------------------
// Gaussian kernel around each MC hit, normalised inside the window: the time-only term carries the 1 / bandwidth factor,
// the (time, charge) terms do not, as in the reference.
__global__ void __launch_bounds__(256) k_pdf_kernel_eval(int time_only, uint32_t nchannels, int ndaq, uint32_t stride,
                                                         const uint32_t *__restrict__ event_hit,
                                                         const float *__restrict__ event_time,
                                                         const float *__restrict__ event_charge,
                                                         const float *__restrict__ mc_time, const float *__restrict__ mc_charge,
                                                         float tmin, float tmax, float qmin, float qmax,
                                                         const float *__restrict__ inv_time_bandwidths,
                                                         const float *__restrict__ inv_charge_bandwidths,
                                                         uint32_t *__restrict__ hitcount, float *__restrict__ time_pdf_values,
                                                         float *__restrict__ charge_pdf_values)
{
    const float invroot2 = 0.70710678118654746f;    // 1 / sqrt(2)
    const float rootPiBy2 = 1.2533141373155001f;    // sqrt(pi / 2)
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nchannels) return;
    const bool hit = event_hit[c] != 0;
    uint32_t count = hitcount[c];
    float tv = 0.0f, qv = 0.0f, et = 0.0f, eq = 0.0f, itb = 0.0f, iqb = 0.0f;
    if (hit) {
        tv = time_pdf_values[c];
        et = event_time[c];
        itb = inv_time_bandwidths[c];
        if (!time_only) { qv = charge_pdf_values[c]; eq = event_charge[c]; iqb = inv_charge_bandwidths[c]; }
    }
    for (int i = 0; i < ndaq; i++) {
        const size_t at = (size_t)i * stride + c;
        const float t = mc_time[at];
        if (!(t >= tmin && t <= tmax)) continue;
        float q = 0.0f;
        if (!time_only) {
            q = mc_charge[at];
            if (!(q >= qmin && q <= qmax)) continue;
        }
        count += 1;
        if (!hit) continue;
        const float arg = (t - et) * itb;
        float norm = tmax - tmin;
        if (itb > 0.0f) {
            const float loarg = (tmin - t) * itb * invroot2;
            const float hiarg = (tmax - t) * itb * invroot2;
            norm = (erff(hiarg) - erff(loarg)) * rootPiBy2;
        }
        if (time_only) {
            const float term = expf(-0.5f * arg * arg) * itb;
            tv += term / norm;
        } else {
            tv += expf(-0.5f * arg * arg) / norm;
            const float qarg = (q - eq) * iqb;
            float qnorm = qmax - qmin;
            if (iqb > 0.0f) {
                const float loarg = (qmin - q) * iqb * invroot2;
                const float hiarg = (qmax - q) * iqb * invroot2;
                qnorm = (erff(hiarg) - erff(loarg)) * rootPiBy2;
            }
            qv += expf(-0.5f * qarg * qarg) / qnorm;
        }
    }
    hitcount[c] = count;
    if (hit) {
        time_pdf_values[c] = tv;
        if (!time_only) charge_pdf_values[c] = qv;
    }
}
