/*
 * TEST INFRASTRUCTURE ONLY.  Force-included (-include) in front of the reference's own
 * src/device.cu and src/MersenneTwister_kernel.cu so that they compile, unmodified and in place,
 * as host C++ (Makefile target oracle/_ref/libref.so).  Nothing of the reference is copied here:
 * this header only supplies the few CUDA names those two files use.
 *
 * max/min/clamp/sign come from the reference's own vec.h (its non-GPU_KERNEL branch), which is
 * why the standard headers are included first: the macros must not reach them.
 */
#ifndef BDPT_REF_SHIM_H
#define BDPT_REF_SHIM_H
#include <cmath>
#include <math.h>
#include <cstdio>
#include <stdio.h>
#include <cstdlib>
#include <stdlib.h>
#include <cstring>

#define __global__
#define __device__

struct ref_dim3 { unsigned x, y, z; };
/* one simulated thread at a time per host thread: the driver sets these before every call */
extern thread_local ref_dim3 threadIdx, blockIdx, blockDim;

struct uchar4 { unsigned char x, y, z, w; };

#define cudaMemcpyToSymbol(sym, src, n) memcpy((sym), (src), (n))
#define __cosf(x) cosf(x)
#define __sinf(x) sinf(x)

#ifndef REF_PLATFORM_LIBM
/* The project's floating-point contract (oracle/bdpt_oracle.c header): cos/sin/pow of a float are
 * the correctly rounded float results, evaluated as (float)f((double)x).  A function-like macro
 * is not expanded inside its own replacement, so ::cos below is the double libm function.  With
 * REF_PLATFORM_LIBM the reference's calls resolve to the platform's float overloads instead
 * (the second build DESIGN.md "Oracle" measures). */
#define cos(x) ((float)::cos((double)(x)))
#define sin(x) ((float)::sin((double)(x)))
#define pow(x, y) ((float)::pow((double)(x), (double)(y)))
#endif

#endif
