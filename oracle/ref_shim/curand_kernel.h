/* curand_kernel.h -- TEST INFRASTRUCTURE.  Stand-in for the CUDA toolkit header of this name, for the host build of
 * the reference's physics (oracle/ref_physics_driver.cc).  The project's own text.
 *
 * A curandState IS the project's per-photon Philox stream (include/chroma_math.h): curand_uniform is its uniform on
 * (0, 1], curand_normal its Box-Muller deviate.  The reference's generator (XORWOW, one state per thread slot) has no
 * counterpart here, so what a comparison through this header pins is everything AROUND the draws -- which statement
 * draws, in what order, how many times -- and not the generator, the word-to-uniform mapping or the normal deviate,
 * which stay the project's own contract on both sides.
 */
#ifndef CHROMA_REF_CURAND_KERNEL_SHIM_H
#define CHROMA_REF_CURAND_KERNEL_SHIM_H

#include "cuda_host_shim.h"
#include "../../include/chroma_math.h"

typedef cm_rng curandState;

static inline float curand_uniform(curandState *s) { return cm_rng_uniform(s); }
static inline float curand_normal(curandState *s) { return cm_rng_normal(s); }

/* sequence = the photon's id, offset = draws already taken */
static inline void curand_init(unsigned long long seed, unsigned long long sequence, unsigned long long offset, curandState *s)
{
    cm_rng_init(s, (uint64_t)seed, (uint64_t)sequence, (uint32_t)offset);
}

#endif /* CHROMA_REF_CURAND_KERNEL_SHIM_H */
