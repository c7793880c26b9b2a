// Device check of the leaf functions of the path kernels themselves (csrc/bdpt_leaf.h, csrc/
// bdpt_math.h), each against a plain statement of what it must return -- never against the function
// under test.  One process; one JSON line per check with the number of inputs, the number of
// mismatches and the first offenders (the input's index in the check's enumeration); exit status 1
// if any check has a mismatch, 2 on a HIP error.  "inputs" is counted by the kernels themselves, so a
// launch that did not run cannot pass; "control_rcp_inrange" runs rcp_rn without its range test over
// all 2^32 patterns and must report mismatches (outside [2^-125, 2^125)): the comparison can fail.
//
//   sincos_tab / sincos_dp   bdpt_sincos_tab (the table of this build: 512 entries, or 256 with
//                            -DBDPT_SC_COARSE=1) and bdpt_sincos_dp on the device over all
//                            268,435,457 x = (2.f*pi) * (f / 2^32), f every float in [1, 2^32]
//                            (tests/native/sincos_check.c's enumeration), against glibc's
//                            (float)sin((double)x) / (float)cos((double)x) computed by the host side
//   sample_record            bdpt_sample_record on the device against its host side, 2^24 seeded
//                            five-tuples and all tuples over the edge values
//   rcp_rn                   all 2^32 patterns against (float)(1.0 / (double)x)
//   rcp_sqrt_rn, sqrt_rn     all 2^31 non-negative patterns, -0 and the negative denormals against
//                            (float)sqrt((double)x) and (float)(1.0 / (double)root); NaN equals NaN
//   div_refraction, div_nee  div_rn_normal on its two stated domains against
//                            (float)((double)a / (double)b)
//   sphere_isect, sphere_roots, sphere_keys
//                            the three forms of the sphere test against the reference's branchy
//                            statement (det < 0: miss; sqrtf; t1 > EPS ? t1 : t2 > EPS ? t2 : 0)
//                            evaluated by the host side, on crafted and seeded inputs
// (double division and sqrt are correctly rounded and 53 >= 2 * 24 + 2, so their rounding to float
// is the correctly rounded float result.)
//
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off leaf_check.hip -o leaf_check
//   hipcc ... -DBDPT_SC_COARSE=1 leaf_check.hip -o leaf_check_coarse      (sincos_tab alone)
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <thread>
#include <vector>

#include "../../gpu_bidirectional_raytracer_amd/csrc/bdpt_device.h"
#include "../../gpu_bidirectional_raytracer_amd/csrc/bdpt_math.h"
#include "../../gpu_bidirectional_raytracer_amd/csrc/bdpt_leaf.h"

#define HIPCK(call)                                                                          \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess) {                                                              \
            fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(e_));                       \
            exit(2);                                                                         \
        }                                                                                    \
    } while (0)

namespace {
constexpr int kThreads = 16;
constexpr int kFirst = 4;
using u64 = unsigned long long;

struct tally { u64 bad, ran; u64 first[kFirst]; };

__device__ __forceinline__ void report(tally* t, u64 id) {
    const u64 k = atomicAdd(&t->bad, 1ull);
    if (k < kFirst) t->first[k] = id;
}
// the inputs this block checks, counted once per block: threads [first, first + 256) below n, x `per`
__device__ __forceinline__ void ran(tally* t, u64 first, u64 n, u64 per = 1) {
    if (threadIdx.x == 0 && first < n) atomicAdd(&t->ran, (n - first < 256 ? n - first : 256ull) * per);
}
__device__ __forceinline__ bool same_f(float a, float b) {            // the bits, NaN equals NaN
    return __float_as_uint(a) == __float_as_uint(b) || (a != a && b != b);
}

int g_failed = 0;
tally* d_tally = nullptr;

void begin() { HIPCK(hipMemset(d_tally, 0, sizeof(tally))); }
double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

void verdict(const char* name, u64 inputs, double t0, tally* dt = nullptr) {
    tally h;
    HIPCK(hipDeviceSynchronize());
    HIPCK(hipMemcpy(&h, dt ? dt : d_tally, sizeof h, hipMemcpyDeviceToHost));
    HIPCK(hipGetLastError());
    if (h.ran != inputs) g_failed = 1;                                // every input was checked by a kernel
    printf("{\"check\": \"%s\", \"inputs\": %llu, \"mismatches\": %llu, \"first\": [", name, h.ran, h.bad);
    for (u64 k = 0; k < h.bad && k < kFirst; k++) printf("%s%llu", k ? ", " : "", h.first[k]);
    printf("], \"seconds\": %.2f}\n", now() - t0);
    fflush(stdout);
    if (h.bad) g_failed = 1;
}

template <typename F>
void parallel(size_t n, F f) {                                        // f(begin, end) on kThreads threads
    std::vector<std::thread> th;
    const size_t per = (n + kThreads - 1) / kThreads;
    for (int k = 0; k < kThreads; k++) {
        const size_t a = k * per, b = a + per < n ? a + per : n;
        if (a < b) th.emplace_back([=] { f(a, b); });
    }
    for (auto& t : th) t.join();
}

float bits_f(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }
uint32_t f_bits(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }

// ---- sincos ----------------------------------------------------------------------------------------
constexpr uint32_t kF0 = 0x3F800000u, kF1 = 0x4F800000u;              // 1.0f and 2^32
constexpr u64 kSincosN = (u64)kF1 - kF0 + 1;                          // 268,435,457

__host__ __device__ inline float sincos_x(uint32_t fb) {
#if defined(__HIP_DEVICE_COMPILE__)
    const float f = __uint_as_float(fb);
#else
    const float f = bits_f(fb);
#endif
    const float u = f / 4294967296.0f;
    return 2.f * 3.14159265358979323846f * u;
}

__global__ void sincos_kernel(u64 i0, u64 n, const float* gs, const float* gc, const double* sintab, tally* tab,
                              tally* dp) {
    const u64 i = blockIdx.x * 256ull + threadIdx.x;
    ran(tab, blockIdx.x * 256ull, n);
    ran(dp, blockIdx.x * 256ull, n);
    if (i >= n) return;
    const float x = sincos_x((uint32_t)(kF0 + i0 + i));
    double s, c;
    bdpt_sincos_tab((double)x, sintab, &s, &c);
    if (!same_f((float)s, gs[i]) || !same_f((float)c, gc[i])) report(tab, i0 + i);
    bdpt_sincos_dp((double)x, &s, &c);
    if (!same_f((float)s, gs[i]) || !same_f((float)c, gc[i])) report(dp, i0 + i);
}

double* upload_sintab() {
    static const double tab[BDPT_SC_N][2] = BDPT_SINCOS_TABLE_INIT;
    double sintab[BDPT_SC_N] = {0};                                   // the kernel's LDS copy: sin(2 pi k / N)
    for (int k = 0; k < (BDPT_SC_N >> BDPT_SC_COARSE); k++) sintab[k] = tab[k << BDPT_SC_COARSE][0];
    double* d;
    HIPCK(hipMalloc(&d, sizeof sintab));
    HIPCK(hipMemcpy(d, sintab, sizeof sintab, hipMemcpyHostToDevice));
    return d;
}

void check_sincos(const double* d_sintab) {
    const double t0 = now();
    constexpr u64 chunk = 1ull << 24;
    std::vector<float> gs(chunk), gc(chunk);
    float *dgs, *dgc;
    tally* d2;                                                        // [0] table, [1] minimax
    HIPCK(hipMalloc(&dgs, chunk * 4));
    HIPCK(hipMalloc(&dgc, chunk * 4));
    HIPCK(hipMalloc(&d2, 2 * sizeof(tally)));
    HIPCK(hipMemset(d2, 0, 2 * sizeof(tally)));
    for (u64 i0 = 0; i0 < kSincosN; i0 += chunk) {
        const u64 n = kSincosN - i0 < chunk ? kSincosN - i0 : chunk;
        parallel(n, [&](size_t a, size_t b) {
            for (size_t i = a; i < b; i++) {
                const float x = sincos_x((uint32_t)(kF0 + i0 + i));
                gs[i] = (float)sin((double)x);
                gc[i] = (float)cos((double)x);
            }
        });
        HIPCK(hipMemcpy(dgs, gs.data(), n * 4, hipMemcpyHostToDevice));
        HIPCK(hipMemcpy(dgc, gc.data(), n * 4, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(sincos_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, i0, n, dgs, dgc, d_sintab,
                           d2, d2 + 1);
        HIPCK(hipDeviceSynchronize());
    }
    verdict(BDPT_SC_COARSE ? "sincos_tab_coarse" : "sincos_tab", kSincosN, t0, d2);
    verdict("sincos_dp", kSincosN, t0, d2 + 1);
    HIPCK(hipFree(dgs));
    HIPCK(hipFree(dgc));
    HIPCK(hipFree(d2));
}

#if !BDPT_SC_COARSE
// ---- sample records --------------------------------------------------------------------------------
__global__ void srec_kernel(u64 i0, u64 n, const float* u, const float* want, const double* sintab, tally* t) {
    const u64 i = blockIdx.x * 256ull + threadIdx.x;
    ran(t, blockIdx.x * 256ull, n);
    if (i >= n) return;
    float out[8];
    bdpt_sample_record(u + 5 * i, sintab, out);
    bool ok = true;
    for (int k = 0; k < 8; k++) ok = ok && same_f(out[k], want[8 * i + k]);
    if (!ok) report(t, i0 + i);
}

void check_sample_record(const double* d_sintab) {
    const double t0 = now();
    static const double tab[BDPT_SC_N][2] = BDPT_SINCOS_TABLE_INIT;
    static double sintab[BDPT_SC_N];
    for (int k = 0; k < BDPT_SC_N; k++) sintab[k] = tab[k][0];
    // the table's values are ((float)y + 1.0f) / 2^32 (MersenneTwister_kernel.cu:108): in [2^-32, 1]
    const float edges[] = {0x1p-32f, 1.f, 1.f - 0x1p-24f, 1.f - 0x1p-23f, 0.5f, 0.25f, 0x1p-24f};
    constexpr int ne = sizeof edges / sizeof edges[0];
    constexpr u64 nedge = (u64)ne * ne * ne * ne * ne, nseed = 1ull << 24, chunk = 1ull << 20;
    std::vector<float> u(5 * chunk), want(8 * chunk);
    float *du, *dw;
    HIPCK(hipMalloc(&du, u.size() * 4));
    HIPCK(hipMalloc(&dw, want.size() * 4));
    begin();
    for (u64 i0 = 0; i0 < nseed + nedge; i0 += chunk) {
        const u64 n = nseed + nedge - i0 < chunk ? nseed + nedge - i0 : chunk;
        parallel(n, [&](size_t a, size_t b) {
            std::mt19937 rng((uint32_t)(20240611u + i0 + a));
            for (size_t i = a; i < b; i++) {
                const u64 id = i0 + i;
                for (int k = 0; k < 5; k++) {
                    if (id < nseed) u[5 * i + k] = ((float)(uint32_t)rng() + 1.0f) / 4294967296.0f;
                    else {
                        u64 q = id - nseed;
                        for (int j = 0; j < k; j++) q /= ne;
                        u[5 * i + k] = edges[q % ne];
                    }
                }
                bdpt_sample_record(&u[5 * i], sintab, &want[8 * i]);
            }
        });
        HIPCK(hipMemcpy(du, u.data(), n * 20, hipMemcpyHostToDevice));
        HIPCK(hipMemcpy(dw, want.data(), n * 32, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(srec_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, i0, n, du, dw, d_sintab, d_tally);
        HIPCK(hipDeviceSynchronize());
    }
    verdict("sample_record", nseed + nedge, t0);
    HIPCK(hipFree(du));
    HIPCK(hipFree(dw));
}

// ---- reciprocals and roots -------------------------------------------------------------------------
__global__ void rcp_kernel(u64 i0, tally* t, tally* control) {
    const u64 i = i0 + blockIdx.x * 256ull + threadIdx.x;
    ran(t, i0 + blockIdx.x * 256ull, 1ull << 32);
    ran(control, i0 + blockIdx.x * 256ull, 1ull << 32);
    if (i >= (1ull << 32)) return;
    const float x = __uint_as_float((unsigned)i);
    const float ref = (float)(1.0 / (double)x);
    if (!same_f(rcp_rn(x), ref)) report(t, i);
    if (!same_f(rcp_rn_inrange(x), ref)) report(control, i);          // the control: no range test
}

constexpr u64 kRootN = (1ull << 31) + (1ull << 23);                   // >= 0, then -0 and the negative denormals

__global__ void root_kernel(u64 i0, tally* rs, tally* sq) {
    const u64 i = i0 + blockIdx.x * 256ull + threadIdx.x;
    ran(rs, i0 + blockIdx.x * 256ull, kRootN);
    ran(sq, i0 + blockIdx.x * 256ull, kRootN);
    if (i >= kRootN) return;
    const float x = __uint_as_float((unsigned)i);                     // i >= 2^31: 0x80000000 + (i - 2^31)
    const float root_ref = (float)sqrt((double)x);
    const float rcp_ref = (float)(1.0 / (double)root_ref);
    float root;
    const float r = rcp_sqrt_rn(x, &root);
    if (!same_f(root, root_ref) || !same_f(r, rcp_ref)) report(rs, i);
    if (!same_f(bdpt_sqrt_rn(x), root_ref)) report(sq, i);
}

void check_reciprocals() {
    double t0 = now();
    tally* d2;
    HIPCK(hipMalloc(&d2, 2 * sizeof(tally)));
    HIPCK(hipMemset(d2, 0, 2 * sizeof(tally)));
    for (u64 i0 = 0; i0 < (1ull << 32); i0 += 1ull << 28)
        hipLaunchKernelGGL(rcp_kernel, dim3(1u << 20), dim3(256), 0, 0, i0, d2, d2 + 1);
    verdict("rcp_rn", 1ull << 32, t0, d2);
    {
        tally h;
        HIPCK(hipMemcpy(&h, d2 + 1, sizeof h, hipMemcpyDeviceToHost));
        printf("{\"check\": \"control_rcp_inrange\", \"inputs\": %llu, \"mismatches\": %llu}\n", h.ran, h.bad);
        if (h.bad == 0) g_failed = 1;
    }
    t0 = now();
    HIPCK(hipMemset(d2, 0, 2 * sizeof(tally)));
    for (u64 i0 = 0; i0 < kRootN; i0 += 1ull << 28)
        hipLaunchKernelGGL(root_kernel, dim3(1u << 20), dim3(256), 0, 0, i0, d2, d2 + 1);
    verdict("rcp_sqrt_rn", kRootN, t0, d2);
    verdict("sqrt_rn", kRootN, t0, d2 + 1);
    HIPCK(hipFree(d2));
}

// ---- div_rn_normal ---------------------------------------------------------------------------------
// Refraction domain: a = Re or Tr, 0 or a multiple of 2^-24 up to 1; b = P or 1 - P in [1/4, 3/4].
// a = k 2^-24 for k = 0..2^24 and -k 2^-24 for k = 1..4 (-0 is outside the function's stated domain,
// "a = +0 or a ... normal": it returns +0 there, and neither Re >= 0 nor Tr = 1 - Re is ever -0).
constexpr u64 kRefrA = (1ull << 24) + 1 + 4;
constexpr int kRefrB = 1024;

__global__ void div_refr_kernel(const float* bs, tally* t) {
    const u64 i = blockIdx.x * 256ull + threadIdx.x;
    ran(t, blockIdx.x * 256ull, kRefrA, kRefrB);
    if (i >= kRefrA) return;
    const float a = i <= (1ull << 24) ? (float)i * 0x1p-24f : -(float)(i - (1ull << 24)) * 0x1p-24f;
    for (int k = 0; k < kRefrB; k++) {
        const float b = bs[k];
        if (!same_f(div_rn_normal(a, b), (float)((double)a / (double)b))) report(t, i * kRefrB + k);
    }
}

// NEE domain: a, b in [2^-60, 2^60].
__global__ void div_pairs_kernel(const float* v, int n, tally* t) {
    const u64 i = blockIdx.x * 256ull + threadIdx.x;
    ran(t, blockIdx.x * 256ull, (u64)n * n);
    if (i >= (u64)n * n) return;
    const float a = v[i / n], b = v[i % n];
    if (!same_f(div_rn_normal(a, b), (float)((double)a / (double)b))) report(t, i);
}
__device__ __forceinline__ u64 mix64(u64 z) {                         // splitmix64's finaliser
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ float nee_value(u64 h) {                   // exponent -60..59, any significand
    const unsigned e = 127u - 60u + (unsigned)((h >> 23) % 120u);
    return __uint_as_float((e << 23) | (unsigned)(h & 0x7FFFFFu));
}
__global__ void div_seeded_kernel(u64 i0, u64 n, tally* t) {
    const u64 i = i0 + blockIdx.x * 256ull + threadIdx.x;
    ran(t, i0 + blockIdx.x * 256ull, n);
    if (i >= n) return;
    const u64 h = mix64(0x9E3779B97F4A7C15ull * (i + 1));
    const float a = nee_value(h), b = nee_value(h >> 32 | h << 32);
    if (!same_f(div_rn_normal(a, b), (float)((double)a / (double)b))) report(t, (1ull << 32) + i);
}

void check_div() {
    double t0 = now();
    std::vector<float> bs;
    const float ends[] = {0.25f, 0.75f, 0.5f};
    for (float e : ends)
        for (float v : {std::nextafterf(e, 0.f), e, std::nextafterf(e, 1.f)})
            if (v >= 0.25f && v <= 0.75f) bs.push_back(v);
    std::mt19937 rng(77);
    while ((int)bs.size() < kRefrB) bs.push_back(bits_f(f_bits(0.25f) + rng() % (f_bits(0.75f) - f_bits(0.25f) + 1)));
    float* dbs;
    HIPCK(hipMalloc(&dbs, kRefrB * 4));
    HIPCK(hipMemcpy(dbs, bs.data(), kRefrB * 4, hipMemcpyHostToDevice));
    begin();
    hipLaunchKernelGGL(div_refr_kernel, dim3((unsigned)((kRefrA + 255) / 256)), dim3(256), 0, 0, dbs, d_tally);
    verdict("div_refraction", kRefrA * kRefrB, t0);
    HIPCK(hipFree(dbs));

    t0 = now();
    std::vector<float> v;                                             // 121 exponents x boundary significands
    for (int e = -60; e <= 60; e++)
        for (uint32_t m : {0u, 1u, 0x400000u, 0x7FFFFFu}) {
            const float x = bits_f(((uint32_t)(127 + e) << 23) | m);
            if (x <= 0x1p60f) v.push_back(x);
        }
    float* dv;
    HIPCK(hipMalloc(&dv, v.size() * 4));
    HIPCK(hipMemcpy(dv, v.data(), v.size() * 4, hipMemcpyHostToDevice));
    const u64 npairs = (u64)v.size() * v.size(), nseed = 1ull << 28;
    begin();
    hipLaunchKernelGGL(div_pairs_kernel, dim3((unsigned)((npairs + 255) / 256)), dim3(256), 0, 0, dv, (int)v.size(), d_tally);
    hipLaunchKernelGGL(div_seeded_kernel, dim3((unsigned)(nseed / 256)), dim3(256), 0, 0, 0ull, nseed, d_tally);
    verdict("div_nee", npairs + nseed, t0);
    HIPCK(hipFree(dv));
}

// ---- the sphere test -------------------------------------------------------------------------------
struct ray_case { float gx, gy, gz, gw, ox, oy, oz, dx, dy, dz, want, t_own; };   // want: the reference's answer

float ref_isect(const ray_case& c) {                                  // SphereIntersectDevice device.cu:80-104
    const float opx = c.gx - c.ox, opy = c.gy - c.oy, opz = c.gz - c.oz;
    const float b = opx * c.dx + opy * c.dy + opz * c.dz;
    float det = b * b - (opx * opx + opy * opy + opz * opz) + c.gw;
    if (det < 0.f) return 0.f;
    det = sqrtf(det);
    float t = b - det;
    if (t > 0.01f) return t;
    t = b + det;
    return t > 0.01f ? t : 0.f;
}

constexpr int kNT = 4, kNM = 20;
struct limits { float t[kNT - 1]; float maxt[kNM]; };

__global__ void sphere_kernel(u64 n, const ray_case* cs, limits lim, tally* t_isect, tally* t_roots, tally* t_keys) {
    const u64 i = blockIdx.x * 256ull + threadIdx.x;
    for (tally* t : {t_isect, t_roots, t_keys}) ran(t, blockIdx.x * 256ull, n);
    if (i >= n) return;
    const ray_case c = cs[i];
    const float4 g = make_float4(c.gx, c.gy, c.gz, c.gw);
    const f3 o = mk(c.ox, c.oy, c.oz), d = mk(c.dx, c.dy, c.dz);
    const float want = c.want;
    if (!same_f(sphere_isect(g, o, d), want)) report(t_isect, i);
    const troots r = sphere_roots(g, o, d), q = roots_of(sphere_det(g, o, d));
    bool ok_r = true, ok_k = true;
    for (int k = 0; k < kNT; k++) {                                   // the closest-hit update
        const float t = k < kNT - 1 ? lim.t[k] : c.t_own;
        const float t_ref = want != 0.f && want < t ? want : t;       // device.cu:106-124
        const float rr = r.t1 > kEps ? r.t1 : r.t2;
        const float t_new = r.t2 > kEps && rr < t ? rr : t;
        ok_r = ok_r && same_f(t_new, t_ref);
        const unsigned kt = key_of(t), nk = umin3(kt, key_of(q.t1), key_of(q.t2));
        ok_k = ok_k && same_f(__uint_as_float(nk + kKeyC), t_ref) && (nk < kt) == (want != 0.f && want < t);
    }
    for (int k = 0; k < kNM; k++) {                                   // the shadow test
        const float m = lim.maxt[k];
        const bool occ_ref = want != 0.f && want < m;                 // device.cu:130-139
        const float rr = r.t1 > kEps ? r.t1 : r.t2;
        ok_r = ok_r && (r.t2 > kEps && rr < m) == occ_ref;
        ok_k = ok_k && (umin2(key_of(q.t1), key_of(q.t2)) < maxt_key(m)) == occ_ref;
    }
    if (!ok_r) report(t_roots, i);
    if (!ok_k) report(t_keys, i);
}

void check_sphere() {
    const double t0 = now();
    const float eps = 0.01f, inf = INFINITY;
    std::vector<ray_case> cs;
    auto head_on = [&](float b, float rr, float px) {                 // o = 0, d = +z, centre (px, 0, b): det = rr - px^2 (+ b^2 - b^2)
        ray_case c = {px, 0.f, b, rr, 0.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 1.f};
        cs.push_back(c);
    };
    std::vector<float> bvals = {0.f, -0.f, bits_f(1), bits_f(0x7FFFFF), 0x1p-126f, std::nextafterf(eps, 0.f), eps,
                                std::nextafterf(eps, 1.f), std::nextafterf(0x1p-23f, 0.f), 0x1p-23f,
                                std::nextafterf(0x1p-23f, 1.f), 0.005f, 1.f, 1e4f, -0.005f, -1.f};
    // det == rad^2 exactly, through (0, 2^-96): below the domain on which the fast root is exact
    std::vector<uint32_t> rrb = {1u, 2u, 0x7FFFFFu, 0x800000u, f_bits(0x1p-96f) - 1, f_bits(0x1p-96f), 0u};
    for (uint32_t b = 1; b < f_bits(0x1p-96f); b += 4093) rrb.push_back(b);
    for (uint32_t w : rrb)
        for (float b : bvals) head_on(b, bits_f(w), 0.f);
    const u64 n_tiny = cs.size();
    // det a negative denormal, b <= EPS: px^2 = 2^-140 (exact), rad^2 = 2^-140 - j 2^-149
    for (int j = 1; j < 512; j++)
        for (float b : {0.f, 0x1p-75f, -0x1p-75f, 0x1p-74f, bits_f(1)}) head_on(b, 0x1p-140f - (float)j * 0x1p-149f, 0x1p-70f);
    const u64 n_negden = cs.size() - n_tiny;
    u64 seen_tiny = 0, seen_negden = 0;                               // the crafted cases are what they claim
    for (const ray_case& c : cs) {
        const float opx = c.gx, b = c.gz, det = b * b - (opx * opx + 0.f * 0.f + b * b) + c.gw;
        seen_tiny += det > 0.f && det < 0x1p-96f;
        seen_negden += det < 0.f && det > -0x1p-126f;
    }
    // seeded ordinary rays and spheres, as tests/test_ikey_rule.py roots_from_spheres makes them
    const u64 n_seed = 1ull << 24, base = cs.size();
    cs.resize(base + n_seed);
    parallel(n_seed, [&](size_t a, size_t b) {
        std::mt19937_64 rng(1000 + a);
        std::uniform_real_distribution<float> pos(-50.f, 150.f), u01(0.f, 1.f), lograd(logf(0.5f), logf(1e4f));
        std::normal_distribution<float> nd;
        for (size_t i = a; i < b; i++) {
            ray_case& c = cs[base + i];
            float dx = nd(rng), dy = nd(rng), dz = nd(rng);
            const float l = sqrtf(dx * dx + dy * dy + dz * dz);
            dx /= l; dy /= l; dz /= l;
            const float rad = expf(lograd(rng));
            c.gx = pos(rng); c.gy = pos(rng); c.gz = pos(rng); c.gw = rad * rad;
            c.ox = pos(rng); c.oy = pos(rng); c.oz = pos(rng);
            if (u01(rng) < 0.2f) { c.ox = c.gx - rad * dx; c.oy = c.gy - rad * dy; c.oz = c.gz - rad * dz; }   // on the surface
            c.dx = dx; c.dy = dy; c.dz = dz;
            c.t_own = u01(rng) < 0.3f ? 1e20f : 0.011f + 300.f * u01(rng);
        }
    });
    parallel(cs.size(), [&](size_t a, size_t b) {
        for (size_t i = a; i < b; i++) cs[i].want = ref_isect(cs[i]);
    });
    u64 hits = 0;
    for (const ray_case& c : cs) hits += c.want != 0.f;
    limits lim = {{1e20f, inf, std::nextafterf(eps, 1.f)},
                  {0.f, -0.f, bits_f(1), -bits_f(1), 1e-30f, 0.005f, 1.f, -1.f, 1e20f, 3.4e38f, -3.4e38f, inf, -inf, NAN, -NAN,
                   1e4f, -1e4f, std::nextafterf(eps, 0.f), eps, std::nextafterf(eps, 1.f)}};
    ray_case* dcs;
    tally* d3;
    HIPCK(hipMalloc(&dcs, cs.size() * sizeof(ray_case)));
    HIPCK(hipMemcpy(dcs, cs.data(), cs.size() * sizeof(ray_case), hipMemcpyHostToDevice));
    HIPCK(hipMalloc(&d3, 3 * sizeof(tally)));
    HIPCK(hipMemset(d3, 0, 3 * sizeof(tally)));
    hipLaunchKernelGGL(sphere_kernel, dim3((unsigned)((cs.size() + 255) / 256)), dim3(256), 0, 0, (u64)cs.size(), dcs, lim,
                       d3, d3 + 1, d3 + 2);
    verdict("sphere_isect", cs.size(), t0, d3);
    verdict("sphere_roots", cs.size(), t0, d3 + 1);
    verdict("sphere_keys", cs.size(), t0, d3 + 2);
    printf("{\"check\": \"sphere_inputs\", \"tiny_det\": %llu, \"tiny_det_cases\": %llu, \"neg_denormal_det\": %llu, "
           "\"neg_denormal_cases\": %llu, \"seeded\": %llu, \"hits\": %llu}\n",
           seen_tiny, n_tiny, seen_negden, n_negden, n_seed, hits);
    HIPCK(hipFree(dcs));
    HIPCK(hipFree(d3));
}
#endif
}  // namespace

int main() {
    const double t0 = now();
    HIPCK(hipMalloc(&d_tally, sizeof(tally)));
    double* d_sintab = upload_sintab();
    check_sincos(d_sintab);
#if !BDPT_SC_COARSE
    check_sample_record(d_sintab);
    check_reciprocals();
    check_div();
    check_sphere();
#endif
    HIPCK(hipDeviceSynchronize());
    printf("{\"check\": \"total\", \"failed\": %d, \"seconds\": %.2f}\n", g_failed, now() - t0);
    HIPCK(hipFree(d_sintab));
    HIPCK(hipFree(d_tally));
    return g_failed;
}
