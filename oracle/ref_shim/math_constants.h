/* math_constants.h -- TEST INFRASTRUCTURE.  Stand-in for the CUDA toolkit header of this name, which
 * chroma/cuda/hybrid_render.cu includes (and uses nothing of), for the host build of oracle/ref_physics_driver.cc.
 * The project's own text: the one constant is pi rounded to float32.
 */
#ifndef CHROMA_REF_MATH_CONSTANTS_SHIM_H
#define CHROMA_REF_MATH_CONSTANTS_SHIM_H

#define CUDART_PI_F 3.14159265358979323846f

#endif /* CHROMA_REF_MATH_CONSTANTS_SHIM_H */
