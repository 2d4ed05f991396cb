// kernels_probe_math.h -- chroma_probe_math: ONE call per element of a single primitive of the numeric contract
// (include/chroma_math.h) as hipcc compiles it for the device, so that tests/test_gpu_math_contract.py can hold it bit for
// bit to the host compiler's build of the same header (the CPU oracle).  The op is a kernel argument: nothing folds at
// compile time.  Every array is read and written as 32-bit WORDS (a float travels as its bits, so that signalling NaNs
// and the integer results of cm_f2i / cm_f2u32 pass untouched).  The numbering is the oracle's (oracle_math 0..18,
// oracle_rng_probe 19..21) and is listed in include/chroma_hip.h.
#pragma once

#define PROBE_MATH_NOPS 22
#define PROBE_MATH_UNIFORM_DRAWS 8
#define PROBE_MATH_NORMAL_DRAWS 4

__global__ void k_probe_math(int op, uint64_t n, const uint32_t *x, const uint32_t *y, const uint32_t *z, uint32_t *out)
{
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (op >= 19) {                                     // six words in: Philox itself, or a stream of draws
        const uint32_t *w = x + 6 * i;
        if (op == 19) {
            uint32_t r[4];
            cm_philox4x32_10(w[0], w[1], w[2], w[3], w[4], w[5], r);
            for (int k = 0; k < 4; k++) out[4 * i + k] = r[k];
            return;
        }
        cm_rng rng;                                     // (seed lo, seed hi, id lo, id hi, stream, start counter)
        cm_rng_init(&rng, (uint64_t)w[0] | ((uint64_t)w[1] << 32), (uint64_t)w[2] | ((uint64_t)w[3] << 32), w[5]);
        rng.stream = w[4];
        if (op == 20) {
            for (int k = 0; k < PROBE_MATH_UNIFORM_DRAWS; k++) out[PROBE_MATH_UNIFORM_DRAWS * i + k] = cm_f2u(cm_rng_uniform(&rng));
        } else {
            for (int k = 0; k < PROBE_MATH_NORMAL_DRAWS; k++) out[PROBE_MATH_NORMAL_DRAWS * i + k] = cm_f2u(cm_rng_normal(&rng));
        }
        return;
    }
    const float a = cm_u2f(x[i]);
    const float b = (op == 7 || op >= 15) ? cm_u2f(y[i]) : 0.0f;
    const float c = (op == 18) ? cm_u2f(z[i]) : 0.0f;
    uint32_t r;
    switch (op) {
    case 0:  r = cm_f2u(cm_logf(a)); break;
    case 1:  r = cm_f2u(cm_expf(a)); break;
    case 2:  r = cm_f2u(cm_sinf(a)); break;
    case 3:  r = cm_f2u(cm_cosf(a)); break;
    case 4:  r = cm_f2u(cm_tanf(a)); break;
    case 5:  r = cm_f2u(cm_asinf(a)); break;
    case 6:  r = cm_f2u(cm_acosf(a)); break;
    case 7:  r = cm_f2u(cm_atan2f(a, b)); break;
    case 8:  r = cm_f2u(cm_sqrtf(a)); break;
    case 9:  r = cm_f2u(cm_u32_to_uniform(x[i])); break;
    case 10: r = cm_f2u(cm_atanf(a)); break;
    case 11: r = cm_f2u(cm_floorf(a)); break;
    case 12: r = cm_f2u(cm_roundf(a)); break;
    case 13: r = (uint32_t)cm_f2i(a); break;
    case 14: r = cm_f2u32(a); break;
    case 15: r = cm_f2u(a / b); break;
    case 16: r = cm_f2u(cm_fminf(a, b)); break;
    case 17: r = cm_f2u(cm_fmaxf(a, b)); break;
    default: r = cm_f2u(cm_fmaf(a, b, c)); break;      // 18
    }
    out[i] = r;
}
