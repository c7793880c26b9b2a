// bdpt_eye.h -- the per-vertex arithmetic of the eye path (device.cu:553-771), stated once for both
// backends, as bdpt_filter.h states the filters': the random-table index, the camera ray, a vertex
// (hit point, normal, dp, nl) and the specular step (mirror and glass).  Two drivers run it: the
// frame kernels bdpt_aov_kernel and bdpt_chain_kernel (bdpt_kernels.hip, whose closest hit -- the
// scalar scene loads and the BVH walk -- is the device's own) and the CPU backend (bdpt_cpu.cpp:
// PathTracer::sample and ::chain, render_aov_cam, the light pass's vertex; Scene::closest is its
// traversal).  bdpt_sides.h says what each side brings.
//
// The exception: bdpt_path_kernel_t and bdpt_light_kernel keep their own text.  The path kernel's
// refraction shares its root and its u with the diffuse branch, its camera ray is formed from LDS
// constants, and every instance is tuned to a register bound; the tests named
// test_path_kernel_of_the_same_context_agrees compare it with this statement.
//
// Numerics: fp32 in the reference's operation order, no contraction, dot() as (x*x' + y*y') + z*z',
// every reciprocal, quotient and root correctly rounded, the fp64 steps of device.cu:565-566 kept.
#pragma once
#include "bdpt_sides.h"

namespace {

// The random-table index of pixel i (= y * W + x), segment `depth` and pass sid, in 32-bit unsigned
// arithmetic (device.cu:562, :612): entries j .. j + 4 are read, j + 4 <= RAND_N - 2.
BDPT_BOTH unsigned eye_rand_index(unsigned i, unsigned depth, unsigned sid) {
    return (26u + i * 25u + depth * 5u + sid) % (kRandN - 5u);
}

// The camera terms of a launch (device.cu:572-592; bdpt_path_args carries the same fields).
struct eye_camera {
    f3 ux, uy, ud, orig;
    float tx, ty, tz, inv_w, inv_h;
    double half_w, half_h;
};

#if !defined(BDPT_KERNEL_SIDE)
// host code only (bdpt_camera is include/bdpt.h's): the terms from a camera and the frame's size,
// with the kernels' float operation order
static inline eye_camera eye_camera_terms(const bdpt_camera& cam, int W, int H) {
    const f3 x = mk(cam.x.x, cam.x.y, cam.x.z), y = mk(cam.y.x, cam.y.y, cam.y.z);
    const f3 dir = mk(cam.dir.x, cam.dir.y, cam.dir.z);
    eye_camera e;
    e.ux = norm(x); e.uy = norm(y); e.ud = norm(dir);
    e.orig = mk(cam.orig.x, cam.orig.y, cam.orig.z);
    e.tx = dot(norm(smul(-1.f, x)), e.orig);              // :584-590
    e.ty = dot(norm(smul(-1.f, y)), e.orig);
    e.tz = dot(smul(-1.f, dir), e.orig);                  // :591-592, no vnorm
    e.inv_w = (float)(14. / W);                           // smallpt_cpu.c:411-412
    e.inv_h = (float)(10.5 / H);
    e.half_w = (double)(e.inv_w * (float)W) / 2.;         // device.cu:565 inv_width*width/2.
    e.half_h = (double)(e.inv_h * (float)H) / 2.;
    return e;
}
#endif

// The camera ray (:562-600) of frame pixel (x, y), as the `fresh` branch of the path kernel forms
// it; u0, u1 are the jitter randoms (+0: the unjittered ray).  1 / w is correctly rounded (the
// reference's (float)(1. / w) has the same bits: double rounding is innocuous for a quotient of floats).
struct eye_ray { f3 o, d; };
BDPT_BOTH eye_ray eye_camera_ray(const eye_camera& c, int x, int y, float u0, float u1) {
    const float kx = (float)(((double)((float)x * c.inv_w) - c.half_w) + (double)(u0 * c.inv_w));
    const float ky = (float)(((double)((float)y * c.inv_h) - c.half_h) + (double)(u1 * c.inv_h));
    const float kz = 10.0f;
    f3 rdir = mk(0.f, 0.f, 0.f);
    rdir = add(rdir, smul(kx, c.ux));
    rdir = add(rdir, smul(ky, c.uy));
    rdir = add(rdir, smul(kz, c.ud));
    const float w = (c.tx * kx + c.ty * ky + c.tz * kz) + 1;
    rdir = smul(flt_rcp(w), rdir);
    return {add(rdir, c.orig), norm(rdir)};
}

// The vertex of a hit at distance t on the sphere about `centre` (:635-643).
struct eye_vertex { f3 hit, normal; float dp; };
BDPT_BOTH eye_vertex eye_vertex_at(f3 o, f3 d, float t, f3 centre) {
    eye_vertex v;
    v.hit = add(o, smul(t, d));
    v.normal = norm(sub(v.hit, centre));
    v.dp = dot(v.normal, d);
    return v;
}
// the normal turned against the ray: (-1 * sign(dp)) * n with sign(dp) = dp > 0 ? 1 : -1, the same
// bits for every n that is not NaN (a NaN's sign is not part of any comparison made here)
BDPT_BOTH f3 eye_nl(f3 normal, float dp) { return dp > 0 ? mk(-normal.x, -normal.y, -normal.z) : normal; }

// One specular step at the vertex (normal, dp) of a sphere of colour cc, for the ray direction d
// and the throughput thr: a mirror (:704-714) reflects; glass (REFR / LITE, :715-770) reflects
// under total internal reflection, and else reflects where reflects(P) says so and transmits where
// not, weighted Re / P or Tr / (1 - P).  sample() and PASS chains pass u < P with the pass's random
// u = rnd[j + 2]; TRANSMIT chains never reflect.
template <class Choice>
BDPT_BOTH void eye_specular(bool mirror, f3 normal, float dp, f3 cc, Choice reflects, f3& d, f3& thr) {
    const f3 refl = sub(d, smul(2.f * dot(normal, d), normal));
    if (!mirror) {
        const f3 nl = eye_nl(normal, dp);
        const float nc = 1.f, nt = 1.5f;
        const bool into = dot(normal, nl) > 0;
        const float nnt = into ? nc / nt : nt / nc;
        const float ddn = dot(d, nl);
        const float cos2t = 1.f - nnt * nnt * (1.f - ddn * ddn);
        if (!(cos2t < 0.f)) {                            // (below 0: total internal reflection)
            // cos2t = 1 - X is 0 or >= 2^-24: the device's core root is exact
            const float kq = (float)(into ? 1 : -1) * (ddn * nnt + flt_sqrt_unit(cos2t));
            const f3 td = norm(sub(smul(nnt, d), smul(kq, normal)));
            const float aa = nt - nc, bb = nt + nc;
            const float R0 = aa * aa / (bb * bb);
            const float c = 1 - (into ? -ddn : dot(td, normal));
            const float Re = R0 + (1 - R0) * c * c * c * c * c;
            const float Tr = 1.f - Re;
            const float P = .25f + .5f * Re;
            const bool reflect = reflects(P);
            // Re or Tr (0 or in [2^-24, 1]: Tr = 1 - Re is a multiple of 2^-24) by P or 1 - P (in
            // [1/4, 3/4]): everything stays normal, the domain of the device's quotient
            const float k = flt_div_normal(reflect ? Re : Tr, reflect ? P : 1.f - P);
            thr = mul(smul(k, thr), cc);
            d = reflect ? refl : td;
            return;
        }
    }
    thr = mul(thr, cc);
    d = refl;
}

}  // namespace

#undef BDPT_BOTH
