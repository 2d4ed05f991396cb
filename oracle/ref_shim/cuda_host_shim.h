/* cuda_host_shim.h -- TEST INFRASTRUCTURE.  The handful of CUDA language and runtime names that the reference's
 * device sources (chroma/cuda/propagate.cu, photon.h, daq.cu and the headers they include) use, given a plain host
 * meaning so that g++ compiles those sources unmodified, from where they lie, into oracle/_ref (oracle/Makefile,
 * oracle/ref_physics_driver.cc; chroma/cuda/pdf.cu with sorting.h through oracle/ref_pdf_driver.cc).  This text is the
 * project's own: nothing here is taken from the reference or from the CUDA toolkit.
 *
 * Execution model of the driver: ONE host thread runs the threads of a block one after the other, thread 0 first,
 * and the blocks of a grid one after the other.  Hence
 *   - __shared__ is `static`: the two kernels that use shared variables (propagate, run_daq_many) set them in
 *     thread 0 and read them in the others, which the order above satisfies;
 *   - __syncthreads() does nothing, and the atomics are the plain read-modify-write they protect.
 *
 * Every system header the reference sources name is included HERE, before the qualifier macros exist (libstdc++
 * spells attributes with some of the same words).
 */
#ifndef CHROMA_REF_CUDA_HOST_SHIM_H
#define CHROMA_REF_CUDA_HOST_SHIM_H

#include <cmath>
#include <cstdlib>
#include <math.h>
#include <float.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define __device__
#define __host__
#define __global__
#define __shared__ static
#define __noinline__ __attribute__((noinline))
#define __forceinline__ inline

/* ---- vector types -------------------------------------------------------------------------------------- */
struct float2 { float x, y; };
struct float3 { float x, y, z; };
struct float4 { float x, y, z, w; };
struct int3 { int x, y, z; };
struct uint3 { unsigned int x, y, z; };
struct uint4 { unsigned int x, y, z, w; };
struct uchar4 { unsigned char x, y, z, w; };

static inline float2 make_float2(float x, float y) { float2 r = {x, y}; return r; }
static inline float3 make_float3(float x, float y, float z) { float3 r = {x, y, z}; return r; }
static inline float4 make_float4(float x, float y, float z, float w) { float4 r = {x, y, z, w}; return r; }
static inline int3 make_int3(int x, int y, int z) { int3 r = {x, y, z}; return r; }
static inline uint3 make_uint3(unsigned int x, unsigned int y, unsigned int z) { uint3 r = {x, y, z}; return r; }
static inline uint4 make_uint4(unsigned int x, unsigned int y, unsigned int z, unsigned int w) { uint4 r = {x, y, z, w}; return r; }
static inline uchar4 make_uchar4(unsigned char x, unsigned char y, unsigned char z, unsigned char w) { uchar4 r = {x, y, z, w}; return r; }

/* ---- the thread's coordinates: set by the driver's launch loops ----------------------------------------- */
struct ref_shim_dim3 { unsigned int x, y, z; };
static ref_shim_dim3 threadIdx = {0, 0, 0}, blockIdx = {0, 0, 0}, blockDim = {1, 1, 1}, gridDim = {1, 1, 1};

static inline void __syncthreads(void) {}

/* ---- atomics: each returns the old value ---------------------------------------------------------------- */
static inline unsigned int atomicAdd(unsigned int *p, unsigned int v) { unsigned int old = *p; *p = old + v; return old; }
static inline int atomicAdd(int *p, int v) { int old = *p; *p = old + v; return old; }
static inline float atomicAdd(float *p, float v) { float old = *p; *p = old + v; return old; }
static inline unsigned int atomicMin(unsigned int *p, unsigned int v) { unsigned int old = *p; if (v < old) *p = v; return old; }
static inline int atomicMin(int *p, int v) { int old = *p; if (v < old) *p = v; return old; }
static inline unsigned int atomicOr(unsigned int *p, unsigned int v) { unsigned int old = *p; *p = old | v; return old; }
static inline int atomicOr(int *p, int v) { int old = *p; *p = old | v; return old; }
/* The exchange fAtomicAdd of hybrid_render.cu is made of.  A driver that wants to know WHERE the running thread adds
 * (the reference has no output for it) sets ref_shim_exch_note: it is told of every exchange of a value other than
 * 0.0f, which in fAtomicAdd is the one that puts `data + what was there` back. */
typedef void (*ref_shim_exch_note_fn)(float *p, float v);
static ref_shim_exch_note_fn ref_shim_exch_note = 0;
static inline float atomicExch(float *p, float v)
{
    float old = *p;
    *p = v;
    if (ref_shim_exch_note && !(v == 0.0f)) ref_shim_exch_note(p, v);
    return old;
}

/* ---- bit casts ------------------------------------------------------------------------------------------ */
static inline float __int_as_float(int i) { float f; memcpy(&f, &i, sizeof f); return f; }
static inline int __float_as_int(float f) { int i; memcpy(&i, &f, sizeof i); return i; }

/* ---- min / max: on floats the device functions are fminf / fmaxf (a NaN operand gives the other operand) -- */
static inline float min(float a, float b) { if (a != a) return b; if (b != b) return a; return (b < a) ? b : a; }
static inline float max(float a, float b) { if (a != a) return b; if (b != b) return a; return (b > a) ? b : a; }
static inline int min(int a, int b) { return (b < a) ? b : a; }
static inline int max(int a, int b) { return (b > a) ? b : a; }
static inline unsigned int min(unsigned int a, unsigned int b) { return (b < a) ? b : a; }
static inline unsigned int max(unsigned int a, unsigned int b) { return (b > a) ? b : a; }

#endif /* CHROMA_REF_CUDA_HOST_SHIM_H */
