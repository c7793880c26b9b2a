// bdpt_sides.h -- what a translation unit brings to the arithmetic that is stated once for both
// backends (bdpt_filter.h: the frame filters; bdpt_eye.h: the eye path's vertices).  This block is
// the one place with two definitions of a name.  A kernel file says so by defining BDPT_KERNEL_SIDE
// before the include: it has bdpt_device.h and bdpt_leaf.h first, so f3 and its operations (mk, add,
// sub, mul, smul, dot, norm), kRandN, the BDPT_DEV_* constants and the fast correctly rounded
// sequences exist, in its device pass and in its host pass alike (which is why the choice cannot be
// __HIP_DEVICE_COMPILE__ alone: the host pass of a kernel file would define f3 twice, and hipcc
// compiles bdpt_cpu.cpp with a device pass that has none of these).  Host code (after <math.h> and
// include/bdpt.h; hipcc or g++) gets the same names here, with 1.f / x, sqrtf, a / b and
// (1.f / sqrtf(dot(v, v))) * v (equal bits: tests/native/hw_exact_check.hip, leaf_check.hip).
// Everything is inlined on both sides.  (The same switch also leaves one host-only function out of
// a kernel file, bdpt_eye.h's eye_camera_terms, which takes include/bdpt.h's camera; it has one
// definition.)
//
// BDPT_BOTH marks a function of the two headers; each of them includes this file first and
// undefines the macro at its end, so it does not reach the including file.
#if defined(BDPT_KERNEL_SIDE)
#define BDPT_BOTH __device__ __forceinline__
#else
#define BDPT_BOTH static inline __attribute__((always_inline))
#endif
#ifndef BDPT_SIDES_H
#define BDPT_SIDES_H

namespace {

#if defined(BDPT_KERNEL_SIDE)
constexpr int kFltDiff = BDPT_DEV_DIFF;
constexpr unsigned kFltCounterCap = BDPT_DEV_COUNTER_CAP;
constexpr float kFltNoiseEps = BDPT_DEV_DNOISE_EPS;
BDPT_BOTH float flt_rcp(float x) { return rcp_rn(x); }
// x in [2^-125, 2^125) proven by the caller
BDPT_BOTH float flt_rcp_inrange(float x) { return rcp_rn_inrange(x); }
// x >= 1 or NaN (1 + a product that is non-negative or NaN): one compare decides between the
// in-range sequence and the library division (+inf, NaN, >= 2^125)
BDPT_BOTH float flt_rcp_ge1(float x) {
    if (__builtin_expect(!(x < 0x1p125f), 0)) return 1.f / x;
    return rcp_rn_inrange(x);
}
BDPT_BOTH float flt_sqrt(float x) { return bdpt_sqrt_rn(x); }
// x is 0 or >= 2^-24 (1 - X with 0 <= X <= 1), proven by the caller: the core root is exact there
BDPT_BOTH float flt_sqrt_unit(float x) { return bdpt_sqrt_rn_core(x); }
// a / b for a = +0 or a, b, a / b and the residual normal, proven by the caller (bdpt_leaf.h)
BDPT_BOTH float flt_div_normal(float a, float b) { return div_rn_normal(a, b); }
#else
constexpr int kFltDiff = BDPT_DIFF;
constexpr unsigned kFltCounterCap = BDPT_COUNTER_CAP;
constexpr float kFltNoiseEps = BDPT_DENOISE_NOISE_EPS;
constexpr unsigned kRandN = BDPT_RAND_N;
struct f3 { float x, y, z; };
BDPT_BOTH f3 mk(float a, float b, float c) { f3 v; v.x = a; v.y = b; v.z = c; return v; }
BDPT_BOTH f3 add(f3 a, f3 b) { return mk(a.x + b.x, a.y + b.y, a.z + b.z); }
BDPT_BOTH f3 sub(f3 a, f3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
BDPT_BOTH f3 mul(f3 a, f3 b) { return mk(a.x * b.x, a.y * b.y, a.z * b.z); }
BDPT_BOTH f3 smul(float k, f3 b) { return mk(k * b.x, k * b.y, k * b.z); }
BDPT_BOTH float dot(f3 a, f3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
BDPT_BOTH f3 norm(f3 v) { return smul(1.f / sqrtf(dot(v, v)), v); }   // vnorm (vec.h:22)
BDPT_BOTH float flt_rcp(float x) { return 1.f / x; }
BDPT_BOTH float flt_rcp_inrange(float x) { return 1.f / x; }
BDPT_BOTH float flt_rcp_ge1(float x) { return 1.f / x; }
BDPT_BOTH float flt_sqrt(float x) { return sqrtf(x); }
BDPT_BOTH float flt_sqrt_unit(float x) { return sqrtf(x); }
BDPT_BOTH float flt_div_normal(float a, float b) { return a / b; }
#endif

}  // namespace
#endif  // BDPT_SIDES_H
