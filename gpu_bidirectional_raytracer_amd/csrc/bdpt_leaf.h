// bdpt_leaf.h -- the leaf device functions of bdpt_kernels.hip: the float3 helpers, the correctly
// rounded reciprocal, square root and quotient with their range tests, sinf/cosf, the sphere test in
// its three forms with the integer keys, and the direction samplers.  Included by bdpt_kernels.hip
// (after bdpt_device.h and bdpt_math.h) and by tests/native/leaf_check.hip, which checks the
// functions themselves on the device against plain statements.
#pragma once

namespace {

// ---------------------------------------------------------------------------------------------
// small float3 helpers with the reference's operation order (vec.h:12-25)
struct f3 { float x, y, z; };
__device__ __forceinline__ f3 mk(float a, float b, float c) { f3 v; v.x = a; v.y = b; v.z = c; return v; }
__device__ __forceinline__ f3 add(f3 a, f3 b) { return mk(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ f3 sub(f3 a, f3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ f3 mul(f3 a, f3 b) { return mk(a.x * b.x, a.y * b.y, a.z * b.z); }
__device__ __forceinline__ f3 smul(float k, f3 b) { return mk(k * b.x, k * b.y, k * b.z); }
__device__ __forceinline__ float dot(f3 a, f3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
// 1.f / x, correctly rounded: v_rcp_f32 + one Newton fma is exactly that for |x| in
// [2^-125, 2^125) (all 2^32 inputs checked on gfx950 by tests/native/hw_exact_check.hip); other
// x take the library division on an exec-masked branch.  rcp_rn_inrange: caller proves the range.
__device__ __forceinline__ float rcp_rn_inrange(float x) {
    const float r = __builtin_amdgcn_rcpf(x);
    return __builtin_fmaf(__builtin_fmaf(-x, r, 1.f), r, r);
}
__device__ __forceinline__ float rcp_rn(float x) {
    const float ax = fabsf(x);
    if (__builtin_expect(!(ax >= 0x1p-125f && ax < 0x1p125f), 0)) return 1.f / x;
    return rcp_rn_inrange(x);
}
// 1.f / sqrtf(x) with both operations correctly rounded, one range test for the pair: for x in
// [2^-96, 2^126) the fast sqrt is exact and its root lies in [2^-48, 2^63), inside rcp_rn's range.
__device__ __forceinline__ float rcp_sqrt_rn(float x, float* root) {
    if (__builtin_expect(!(x >= 0x1p-96f && x < 0x1p126f), 0)) {
        *root = sqrtf(x);
        return 1.f / *root;
    }
    *root = bdpt_sqrt_rn_core(x);
    return rcp_rn_inrange(*root);
}

// a / b, correctly rounded, for a = +0 or a, b, a/b and the residual normal: one Markstein step on
// the exact reciprocal, y = RN(1/b), q = RN(a y), r = a - q b (exact by fma), RN(q + r y).  Checked
// on every pair of fp32 significands (2^46 pairs, 0 mismatches, scripts/div_check.hip); correct
// rounding of a quotient of normal numbers depends on the significands only.  The refraction
// weight divides Re or Tr (0 or in [2^-24, 1]: Tr = 1 - Re is a multiple of 2^-24) by P or 1 - P
// (in [1/4, 3/4]), so everything stays normal; a = +0 gives q = r = +0.
__device__ __forceinline__ float div_rn_normal(float a, float b) {
    const float y = rcp_rn_inrange(b);
    const float q = a * y;
    const float r = __builtin_fmaf(-q, b, a);
    return __builtin_fmaf(r, y, q);
}
__device__ __forceinline__ f3 norm(f3 v) {
    float root;
    return smul(rcp_sqrt_rn(dot(v, v), &root), v);             // one range test (above)
}
__device__ __forceinline__ f3 cross(f3 a, f3 b) {
    return mk(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}
__device__ __forceinline__ bool iszero3(f3 v) { return v.x == 0.f && v.y == 0.f && v.z == 0.f; }

constexpr float kEps = 0.01f;                              // geom.h:6 EPSILON
constexpr float kPi = 3.14159265358979323846f;             // geom.h:7 FLOAT_PI
constexpr unsigned kRandN = BDPT_DEV_RAND_N;

// the table of bdpt_sincos_tab in device memory (copied to LDS by the path kernel)
__device__ const double bdpt_sincos_table_dev[BDPT_SC_N][2] = BDPT_SINCOS_TABLE_INIT;

// sinf/cosf with correctly-rounded semantics: fp64 sincos rounded once to fp32 (bdpt_math.h),
// table-driven when the caller has the sin(2pi k/N) table in LDS.
// The choice is a template argument, not a null test on `tab`: the compiler cannot prove an
// LDS-derived pointer non-null, and the dead minimax path then kept its fp64 coefficients in
// ~20 VGPRs across the whole path loop.
template <bool TAB>
__device__ __forceinline__ void sincos_cr(float x, float* s, float* c, const double* tab) {
    double sd, cd;
    if constexpr (TAB) bdpt_sincos_tab((double)x, tab, &sd, &cd);
    else bdpt_sincos_dp((double)x, &sd, &cd);
    *s = (float)sd;
    *c = (float)cd;
}

// SphereIntersectDevice device.cu:80-104 (g = {p.x, p.y, p.z, rad*rad}), branch-free.
// For 0 <= det < 2^-96 the root is not correctly rounded, but it is < 2^-47: then either
// |b| >= 2^-23 and fl(b -+ root) == b == fl(b -+ sqrtf(det)), or both roots are < EPSILON and the
// test returns 0 -- the result equals the reference's for every det.
__device__ __forceinline__ float sphere_isect(float4 g, f3 o, f3 d) {
    f3 op = mk(g.x - o.x, g.y - o.y, g.z - o.z);
    float b = dot(op, d);
    float det = b * b - dot(op, op) + g.w;
    const float s = bdpt_sqrt_rn_core(det);
    const float t1 = b - s, t2 = b + s;
    const float r = t1 > kEps ? t1 : (t2 > kEps ? t2 : 0.f);
    return det < 0.f ? 0.f : r;
}

// The two roots of the same test, t1 <= t2 (fl is monotone and the root is >= 0; both NaN for a
// negative det).  With r = t1 > EPS ? t1 : t2, the reference's hit (t1 > EPS ? t1 : t2 > EPS ?
// t2 : miss) is "r if t2 > EPS": when t1 > EPS, t2 >= t1 > EPS too.  So the closest-hit update is
// `t2 > EPS && r < t` and the shadow test `t2 > EPS && r < maxt`: one select fewer than with a
// +inf miss encoding (two compares and a select instead of two selects and a compare).
// The reference's `det < 0 -> miss` needs no test of its own (+2.7 % measured): a negative normal
// det gives a NaN root (bdpt_sqrt_rn_core), so t1, t2, r are NaN and t2 > EPS fails; so does a
// generated NaN det.  A negative denormal det may give a root of -0 (v_sqrt_f32 flushes it), so
// r = b -- but then b <= EPS, a miss again: if b > EPS, then fl(b*b) >= 1e-4 and X = fl(b*b - oo)
// is either > 0 (oo < b*b/2; then det >= X > 0) or a multiple of 2^-38 (ulp(oo) >= 2^-38), and
// det = fl(X + r*r) is then >= 0, <= -2^-39, or a nonzero multiple of ulp(r*r) >= 2^-83 -- never
// in (-2^-126, 0).  (det is never -0: fl(b*b) is not -0.)
struct troots { float t1, t2; };
__device__ __forceinline__ troots sphere_roots(float4 g, f3 o, f3 d) {
    f3 op = mk(g.x - o.x, g.y - o.y, g.z - o.z);
    float b = dot(op, d);
    float det = b * b - dot(op, op) + g.w;
    const float s = bdpt_sqrt_rn_core(det);
    return {b - s, b + s};
}
// The same test in two steps, so that a wave can stop after `det` when no lane's det is >= 0 (or
// NaN): every such lane misses (the reference returns 0 for det < 0, device.cu:95), so the root,
// its correction, the two roots and the selects of that sphere are skipped for the whole wave.
// Specialised kernels use it for the non-wall spheres (radius < 1000: for a wall every line hits),
// where most waves' rays all miss the sphere's line.
struct tdet { float b, det; };
__device__ __forceinline__ tdet sphere_det(float4 g, f3 o, f3 d) {
    f3 op = mk(g.x - o.x, g.y - o.y, g.z - o.z);
    float b = dot(op, d);
    return {b, b * b - dot(op, op) + g.w};
}
__device__ __forceinline__ troots roots_of(tdet q) {
    const float s = bdpt_sqrt_rn_core(q.det);
    return {q.b - s, q.b + s};
}
// Hit distances as unsigned keys (BDPT_IKEY; specialised kernels): key(x) = bits(x) - kKeyC mod
// 2^32 with kKeyC = bits(EPSILON) + 1.  For x > EPSILON (+inf included) key(x) <= key(+inf) and
// the key increases with x; every x <= EPSILON (+0 included), every NaN and every negative float
// maps above key(+inf) (the subtraction wraps, or the sign bit survives it).  t1 <= t2 (or both
// NaN), so min(key(t1), key(t2)) is key(t1 > EPS ? t1 : t2) when that value is > EPS and a miss
// key otherwise: the closest-hit update becomes one min3 with the running key (plus the compare
// and select of the index), and the shadow test one unsigned compare against key(maxt) (0 when
// maxt <= EPS or NaN: nothing occludes, as in the float test).
// (The rule is checked on edge values and random roots by tests/test_ikey_rule.py.)
constexpr unsigned kKeyC = 0x3C23D70Bu;                      // bits(0.01f) + 1
__device__ __forceinline__ unsigned key_of(float x) { return __float_as_uint(x) - kKeyC; }
__device__ __forceinline__ unsigned umin2(unsigned a, unsigned b) { return a < b ? a : b; }
// one v_min3_u32 (left to itself the compiler compares min(b, c) with a and keeps a separate min:
// two half-rate v_min_u32, and the kernels ran 0.5-1 % slower than without keys)
__device__ __forceinline__ unsigned umin3(unsigned a, unsigned b, unsigned c) {
    unsigned r;
    asm("v_min3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__device__ __forceinline__ unsigned maxt_key(float maxt) { return maxt > kEps ? key_of(maxt) : 0u; }

// UniformSampleSphereDevice device.cu:157-165, with s, c = sinf, cosf(2 pi u2) given
__device__ __forceinline__ f3 uniform_sphere_sc(float u1, float s, float c) {
    const float zz = 1.f - 2.f * u1;
    const float q = 1.f - zz * zz;
    const float r = bdpt_sqrt_rn_core(0.f > q ? 0.f : q);   // q is 0 or >= 2^-24: core is exact
    return mk(r * c, r * s, zz);
}
template <bool TAB = false>
__device__ __forceinline__ f3 uniform_sphere(float u1, float u2, const double* tab = nullptr) {
    const float phi = 2.f * kPi * u2;
    float s, c;
    sincos_cr<TAB>(phi, &s, &c, tab);
    return uniform_sphere_sc(u1, s, c);
}

// Cosine-weighted direction about w (device.cu:676-699; also :190-212 and :357-380).
template <bool TAB = false>
__device__ __forceinline__ f3 cosine_dir(f3 w, float u_phi, float u_r2, const double* tab = nullptr) {
    const float r1 = 2.f * kPi * u_phi;
    const float r2 = u_r2;
    const float r2s = bdpt_sqrt_rn_core(r2);                 // r2 = d_Rand value >= 2^-32
    f3 a = fabsf(w.x) > .1f ? mk(0.f, 1.f, 0.f) : mk(1.f, 0.f, 0.f);
    const f3 uc = cross(a, w);                                // |uc|^2 >= 0.01 by the choice of a
    f3 u = smul(rcp_rn_inrange(bdpt_sqrt_rn_core(dot(uc, uc))), uc);   // 0.1 <= |uc| <= 1
    f3 v = cross(w, u);
    float s, c;
    sincos_cr<TAB>(r1, &s, &c, tab);
    u = smul(c * r2s, u);
    v = smul(s * r2s, v);
    f3 nd = add(u, v);
    w = smul(bdpt_sqrt_rn_core(1 - r2), w);                   // 1 - r2 is 0 or >= 2^-24
    return add(nd, w);
}

// The rest of cosine_dir once u = normalize(cross(a, w)) and r2s = sqrt(r2) are known (the path
// kernel computes those two on a path shared with refraction): the same operations in the same
// order as cosine_dir.
// (s, c = sinf, cosf(2 pi u_phi) given: cosine_tail_sc)
__device__ __forceinline__ f3 cosine_tail_sc(f3 w, f3 u, float s, float c, float u_r2, float r2s) {
    f3 v = cross(w, u);
    u = smul(c * r2s, u);
    v = smul(s * r2s, v);
    f3 nd = add(u, v);
    w = smul(bdpt_sqrt_rn_core(1 - u_r2), w);                // 1 - r2 is 0 or >= 2^-24
    return add(nd, w);
}
template <bool TAB = false>
__device__ __forceinline__ f3 cosine_tail(f3 w, f3 u, float u_phi, float u_r2, float r2s,
                                          const double* tab = nullptr) {
    const float r1 = 2.f * kPi * u_phi;
    float s, c;
    sincos_cr<TAB>(r1, &s, &c, tab);
    return cosine_tail_sc(w, u, s, c, u_r2, r2s);
}

}  // namespace
