/* cuComplex.h -- TEST INFRASTRUCTURE.  Stand-in for the CUDA toolkit header of this name, as far as the reference's
 * thin-film model uses it (chroma/cuda/photon.h:410-514, chroma/cuda/cx.h), for the host build of
 * oracle/ref_physics_driver.cc.  Written on its own; it includes neither the oracle nor the engine.
 *
 * Sums, differences and products are the textbook ones.  The quotient and the modulus are the SCALED forms the
 * toolkit documents: the quotient divides both operands by |Re b| + |Im b| before it forms b's squared modulus, and
 * the modulus is larger * sqrt(1 + (smaller / larger)^2), with larger + smaller for a zero or non-finite operand.
 * The scaling decides the last bits and where an overflow turns into Inf or NaN, so it is part of what is compared.
 */
#ifndef CHROMA_REF_CUCOMPLEX_SHIM_H
#define CHROMA_REF_CUCOMPLEX_SHIM_H

#include "cuda_host_shim.h"

typedef float2 cuFloatComplex;

static inline cuFloatComplex make_cuFloatComplex(float r, float i) { cuFloatComplex c; c.x = r; c.y = i; return c; }
static inline float cuCrealf(cuFloatComplex a) { return a.x; }
static inline float cuCimagf(cuFloatComplex a) { return a.y; }
static inline cuFloatComplex cuConjf(cuFloatComplex a) { return make_cuFloatComplex(a.x, -a.y); }

static inline cuFloatComplex cuCaddf(cuFloatComplex a, cuFloatComplex b) { return make_cuFloatComplex(a.x + b.x, a.y + b.y); }
static inline cuFloatComplex cuCsubf(cuFloatComplex a, cuFloatComplex b) { return make_cuFloatComplex(a.x - b.x, a.y - b.y); }

static inline cuFloatComplex cuCmulf(cuFloatComplex a, cuFloatComplex b)
{
    return make_cuFloatComplex((a.x * b.x) - (a.y * b.y), (a.x * b.y) + (a.y * b.x));
}

static inline cuFloatComplex cuCdivf(cuFloatComplex a, cuFloatComplex b)
{
    float scale = fabsf(b.x) + fabsf(b.y);
    float inv = 1.0f / scale;
    float ar = a.x * inv, ai = a.y * inv;
    float br = b.x * inv, bi = b.y * inv;
    float mod2 = (br * br) + (bi * bi);
    float inv2 = 1.0f / mod2;
    return make_cuFloatComplex(((ar * br) + (ai * bi)) * inv2, ((ai * br) - (ar * bi)) * inv2);
}

static inline float cuCabsf(cuFloatComplex a)
{
    float re = fabsf(a.x), im = fabsf(a.y);
    float big = (re > im) ? re : im;
    float small = (re > im) ? im : re;
    float q = small / big;
    float r = big * sqrtf(1.0f + q * q);
    if (big == 0.0f || big > FLT_MAX || small > FLT_MAX)
        r = big + small;
    return r;
}

#endif /* CHROMA_REF_CUCOMPLEX_SHIM_H */
