// bdpt_cpu.cpp -- the host (CPU) backend of the C-ABI: a render context that runs the reference's
// render path on the CPU cores, selected with device = BDPT_DEVICE_CPU in bdpt_create.  It is the
// product's answer to "smallpt_cpu.c CPU path" configs (BASELINE.json configs[0]) and to a machine
// without a GPU; it is not a fallback -- a GPU context never routes here.
//
// Same floating-point contract as the HIP kernels: IEEE fp32 with no contraction
// (built with -ffp-contract=off), correctly rounded division and sqrt, the fp64 camera steps of
// device.cu:565-566, sin/cos as (float)f((double)x).  So its frames equal the GPU's bit for bit.
// Work is spread over threads by pixel row (each pixel renders its passes in order, as the
// running mean requires).
//
// The frame services (denoisers, reprojection, noise estimate) take what a pixel or a tap computes
// from bdpt_filter.h, the one statement of it that the HIP kernels run too; this file is the host's
// driver of it: rows over threads, plain arrays instead of packed records.  The eye path's vertices
// (camera ray, hit point and normal, mirror and glass) are bdpt_eye.h's in the same way, between
// this file's own traversal (Scene).
#include "bdpt_cpu.h"

#include <math.h>
#include <sched.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <thread>
#include <vector>

#include "bdpt_eye.h"
#include "bdpt_filter.h"

namespace {

constexpr float kEps = 0.01f;                              // geom.h:6 EPSILON
constexpr float kPi = 3.14159265358979323846f;             // geom.h:7 FLOAT_PI

// the operator spelling of bdpt_sides.h's f3 operations, for the traversal and the light sampling
inline f3 operator+(f3 a, f3 b) { return add(a, b); }
inline f3 operator-(f3 a, f3 b) { return sub(a, b); }
inline f3 operator*(f3 a, f3 b) { return mul(a, b); }
inline f3 operator*(float k, f3 b) { return smul(k, b); }
inline f3 cross(f3 a, f3 b) { return mk(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
inline bool zero(f3 v) { return v.x == 0.f && v.y == 0.f && v.z == 0.f; }
inline f3 of(const bdpt_vec& v) { return mk(v.x, v.y, v.z); }
inline float fsin(float x) { return (float)sin((double)x); }
inline float fcos(float x) { return (float)cos((double)x); }

// Scene in structure-of-arrays form for the traversal loops.
struct Scene {
    unsigned n = 0;
    std::vector<float> px, py, pz, rad;
    std::vector<unsigned char> emissive;
    std::vector<bdpt_sphere> s;
    void load(const bdpt_sphere* sp, unsigned count) {
        n = count;
        s.assign(sp, sp + count);
        px.resize(n); py.resize(n); pz.resize(n); rad.resize(n); emissive.resize(n);
        for (unsigned i = 0; i < n; i++) {
            px[i] = sp[i].p.x; py[i] = sp[i].p.y; pz[i] = sp[i].p.z; rad[i] = sp[i].rad;
            emissive[i] = !zero(of(sp[i].e));
        }
    }
    // SphereIntersectDevice device.cu:80-104: 0 = miss
    float hit(unsigned i, f3 o, f3 d) const {
        const f3 op = mk(px[i], py[i], pz[i]) - o;
        const float b = dot(op, d);
        float det = b * b - dot(op, op) + rad[i] * rad[i];
        if (det < 0.f) return 0.f;
        det = sqrtf(det);
        const float t1 = b - det;
        if (t1 > kEps) return t1;
        const float t2 = b + det;
        return t2 > kEps ? t2 : 0.f;
    }
    // IntersectDevice device.cu:106-124: scan from the last sphere down, `<` keeps ties
    bool closest(f3 o, f3 d, float* t, unsigned* id) const {
        *t = 1e20f;
        for (unsigned i = n; i--;) {
            const float h = hit(i, o, d);
            if (h != 0.f && h < *t) { *t = h; *id = i; }
        }
        return *t < 1e20f;
    }
    // IntersectPDevice / IntersectPVacuumDevice device.cu:126-154
    bool occluded(f3 o, f3 d, float maxt, bool vacuum) const {
        for (unsigned i = n; i--;) {
            const float h = hit(i, o, d);
            if (h != 0.f && h < maxt && !(vacuum && emissive[i])) return true;
        }
        return false;
    }
};

// UniformSampleSphereDevice device.cu:157-165
f3 sphere_point(float u1, float u2) {
    const float zz = 1.f - 2.f * u1;
    const float q = 1.f - zz * zz;
    const float r = sqrtf(0.f > q ? 0.f : q);
    const float phi = 2.f * kPi * u2;
    return mk(r * fcos(phi), r * fsin(phi), zz);
}

// cosine-weighted direction about w (device.cu:190-212, 357-380, 676-699)
f3 cosine_dir(f3 w, float u_phi, float r2) {
    const float r1 = 2.f * kPi * u_phi;
    const float r2s = sqrtf(r2);
    const f3 a = fabsf(w.x) > .1f ? mk(0.f, 1.f, 0.f) : mk(1.f, 0.f, 0.f);
    f3 u = norm(cross(a, w));
    f3 v = cross(w, u);
    u = (fcos(r1) * r2s) * u;
    v = (fsin(r1) * r2s) * v;
    return (u + v) + sqrtf(1 - r2) * w;
}

unsigned to_int8(float v, const float* thr) {                // toInt (vec.h:34) by threshold search
    unsigned k = 0;
    for (unsigned step = 128; step > 0; step >>= 1)
        if (v >= thr[k + step]) k += step;
    return k;
}

// n colours as RGBA8 through the gamma thresholds
void to_rgba(const float* thr, const bdpt_vec* col, size_t n, unsigned char* rgba) {
    for (size_t i = 0; i < n; i++) {
        rgba[4 * i] = (unsigned char)to_int8(col[i].x, thr);
        rgba[4 * i + 1] = (unsigned char)to_int8(col[i].y, thr);
        rgba[4 * i + 2] = (unsigned char)to_int8(col[i].z, thr);
        rgba[4 * i + 3] = 0;
    }
}

inline bdpt_vec to_vec(f3 v) { return {v.x, v.y, v.z}; }

int worker_count() {
    if (const char* e = getenv("BDPT_CPU_THREADS")) {
        const int t = atoi(e);
        if (t > 0) return t;
    }
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof set, &set) == 0) return CPU_COUNT(&set) > 0 ? CPU_COUNT(&set) : 1;
    const unsigned h = std::thread::hardware_concurrency();
    return h ? (int)h : 1;
}

template <class F>
void parallel_rows(int y0, int y1, int threads, F body) {
    std::atomic<int> next(y0);
    auto run = [&] {
        for (int y; (y = next.fetch_add(1)) < y1;) body(y);
    };
    const int nt = threads < y1 - y0 ? threads : (y1 - y0 > 0 ? y1 - y0 : 1);
    std::vector<std::thread> pool;
    for (int t = 1; t < nt; t++) pool.emplace_back(run);
    run();
    for (std::thread& t : pool) t.join();
}

}  // namespace

struct bdpt_cpu_ctx {
    int W = 0, H = 0;
    Scene scene;
    bdpt_camera cam{};
    bool cam_set = false, rand_ready = false;
    uint32_t params[4 * BDPT_MT_RNG_COUNT];
    std::vector<float> rnd;
    std::vector<bdpt_lightpath> lp;
    std::vector<bdpt_vec> colors;
    std::vector<unsigned> counter;
    std::vector<unsigned char> pixels;
    float thr[256];
    int shard = 0, nshards = 1, band_rows = 8;
    int threads = 1;
    // history of bdpt_reproject (include/bdpt.h): colour, weight and guides per pixel under hcam
    // and the spheres hsph; has_hist says that one is stored; follow: bdpt_history_follow's switch
    bool has_hist = false, follow = false;
    bdpt_camera hcam{};
    std::vector<bdpt_sphere> hsph;
    std::vector<bdpt_vec> hc, gpos;
    std::vector<float> hm;
    std::vector<int> gid;
    // mark of bdpt_noise_estimate (include/bdpt.h): one 16-byte record per pixel, allocated on
    // first use; empty while no mark was ever stored
    struct NoiseMark { bdpt_vec c; unsigned n; };
    std::vector<NoiseMark> mark;
    std::vector<unsigned> last_pending;   // per tile, of the last estimate (empty: none made yet)
};

extern "C" void bdpt_gamma_thresholds(float thr[256]);

bdpt_cpu_ctx* bdpt_cpu_create(const bdpt_sphere* spheres, unsigned n, int W, int H, const uint32_t* params) {
    bdpt_cpu_ctx* c = new (std::nothrow) bdpt_cpu_ctx();
    if (!c) return nullptr;
    c->W = W; c->H = H;
    c->scene.load(spheres, n);
    memcpy(c->params, params, sizeof c->params);
    const size_t np = (size_t)W * H;
    c->lp.assign(BDPT_LIGHT_POINTS, bdpt_lightpath{});        // zero-initialised (Appendix A.4)
    c->colors.assign(np, bdpt_vec{0.f, 0.f, 0.f});
    c->counter.assign(np, 0u);
    c->pixels.assign(4 * np, 0);
    bdpt_gamma_thresholds(c->thr);
    c->threads = worker_count();
    return c;
}

void bdpt_cpu_destroy(bdpt_cpu_ctx* c) { delete c; }

// (the calls that rewrite the accumulation other than path passes clear the noise estimate's mark)
void bdpt_cpu_set_scene(bdpt_cpu_ctx* c, const bdpt_sphere* spheres, unsigned n) {
    c->scene.load(spheres, n);
    bdpt_cpu_noise_clear(c);
}
void bdpt_cpu_set_camera(bdpt_cpu_ctx* c, const bdpt_camera* cam) {
    c->cam = *cam;
    c->cam_set = true;
    bdpt_cpu_noise_clear(c);
}
void bdpt_cpu_reset_accum(bdpt_cpu_ctx* c) {
    std::fill(c->counter.begin(), c->counter.end(), 0u);
    bdpt_cpu_noise_clear(c);
}
void bdpt_cpu_set_shard(bdpt_cpu_ctx* c, int shard, int nshards, int band_rows) {
    c->shard = shard; c->nshards = nshards; c->band_rows = band_rows;
}
int bdpt_cpu_threads(const bdpt_cpu_ctx* c) { return c->threads; }

// seedMTGPU(seed) + RandomGPU (MersenneTwister_kernel.cu:39-110): 4096 MT607 lanes, lane-major.
void bdpt_cpu_generate_rand(bdpt_cpu_ctx* c, unsigned seed) {
    c->rnd.resize(kRandN);
    float* out = c->rnd.data();
    const uint32_t* prm = c->params;
    parallel_rows(0, BDPT_MT_RNG_COUNT / 64, c->threads, [&](int blk) {
        for (int tid = blk * 64; tid < blk * 64 + 64; tid++) {
            const uint32_t a = prm[4 * tid], mb = prm[4 * tid + 1], mc = prm[4 * tid + 2];
            uint32_t mt[19];
            mt[0] = seed;
            for (int s = 1; s < 19; s++) mt[s] = 1812433253u * (mt[s - 1] ^ (mt[s - 1] >> 30)) + (uint32_t)s;
            for (int k = 0, s = 0; k < BDPT_N_PER_RNG; k++, s = s == 18 ? 0 : s + 1) {
                const int s1 = s == 18 ? 0 : s + 1, sm = s + 9 >= 19 ? s + 9 - 19 : s + 9;
                uint32_t y = (mt[s] & 0xFFFFFFFEu) | (mt[s1] & 0x1u);
                y = mt[sm] ^ (y >> 1) ^ ((y & 1u) ? a : 0u);
                mt[s] = y;
                y ^= y >> 12;
                y ^= (y << 7) & mb;
                y ^= (y << 15) & mc;
                y ^= y >> 18;
                out[tid + k * BDPT_MT_RNG_COUNT] = ((float)y + 1.0f) / 4294967296.0f;
            }
        }
    });
    c->rand_ready = true;
}

// UpdateRendering2 smallpt_cpu.c:311-359: GetRayKernel + RadianceLightTracingKernel per emitter,
// in sphere order (a later light overwrites the VLPs an earlier one wrote).
void bdpt_cpu_light_pass(bdpt_cpu_ctx* c, int current_sample) {
    bdpt_cpu_generate_rand(c, (unsigned)(current_sample * 5));
    const Scene& sc = c->scene;
    const float* rnd = c->rnd.data();
    for (unsigned li = 0; li < sc.n; li++) {
        if (!sc.emissive[li]) continue;
        const bdpt_sphere L = sc.s[li];
        parallel_rows(0, BDPT_LIGHT_POINTS / 64, c->threads, [&](int blk) {
            for (int ind = blk * 64; ind < blk * 64 + 64; ind++) {
                const unsigned i = (unsigned)(current_sample * 5 + ind * 4) % (kRandN - 4u), j = i + 2;
                const f3 spt = L.rad * sphere_point(rnd[j], rnd[i]) + of(L.p);
                const f3 o = spt, d = cosine_dir(norm(spt - of(L.p)), rnd[i + 1], rnd[j + 1]);
                f3 thr = 0.25f * of(L.e);
                float t;
                unsigned id = 0;
                bdpt_lightpath& out = c->lp[ind];
                if (!sc.closest(o, d, &t, &id)) {                      // escaped (:279-292)
                    const f3 nor = (float)(-1. / (double)L.rad) * (o - of(L.p)), hr = 0.5f * of(L.e);
                    out.hp = {o.x, o.y, o.z}; out.rad = {hr.x, hr.y, hr.z}; out.nl = {nor.x, nor.y, nor.z};
                    continue;
                }
                const bdpt_sphere& O = sc.s[id];
                if (sc.emissive[id]) continue;                          // :296-298
                const eye_vertex p = eye_vertex_at(o, d, t, of(O.p));
                const f3 h = p.hit, nl = eye_nl(p.normal, p.dp);
                if (O.refl != BDPT_DIFF) continue;                      // DEPTH = 1: no store
                const float tol = (float)0.0001;                         // VecMultiply :10-42
                float* tv[3] = {&thr.x, &thr.y, &thr.z};
                const float cv[3] = {O.c.x, O.c.y, O.c.z};
                for (int k = 0; k < 3; k++) {
                    if (*tv[k] != 0.f && cv[k] != 0.f) {
                        const float m = *tv[k] * cv[k];
                        if (!(m <= tol || *tv[k] == m)) *tv[k] = m;
                    } else {
                        *tv[k] = 0.f;
                    }
                }
                out.hp = {h.x, h.y, h.z}; out.rad = {thr.x, thr.y, thr.z}; out.nl = {nl.x, nl.y, nl.z};
            }
        });
    }
}

namespace {
// RadiancePathTracingKernel device.cu:553-771 for one (pixel, pass): the radiance of one eye path.
struct PathTracer {
    const Scene& sc;
    const float* rnd;
    const bdpt_lightpath* lp;
    eye_camera cam;

    PathTracer(const bdpt_cpu_ctx* c) : PathTracer(c, c->cam) {}
    // under a camera other than the context's (the history's, bdpt_cpu_history_write)
    PathTracer(const bdpt_cpu_ctx* c, const bdpt_camera& cm)
        : sc(c->scene), rnd(c->rnd.data()), lp(c->lp.data()), cam(eye_camera_terms(cm, c->W, c->H)) {}

    // SampleLightsDevice device.cu:457-542: NEE to every emitter + one VLP, blended 1/2
    f3 lights(f3 h, f3 nl, unsigned j, const bdpt_lightpath& v) const {
        f3 res = mk(0.f, 0.f, 0.f);
        for (unsigned i = 0; i < sc.n; i++) {
            if (!sc.emissive[i]) continue;
            const bdpt_sphere& L = sc.s[i];
            const f3 usp = sphere_point(rnd[j + 3], rnd[j + 4]);
            f3 sd = (L.rad * usp + of(L.p)) - h;
            const float len = sqrtf(dot(sd, sd));
            sd = (1.f / len) * sd;
            float wo = dot(sd, usp);
            if (wo > 0.f) continue;
            wo = -wo;
            const float wi = dot(sd, nl);
            if (wi > 0.f && !sc.occluded(h, sd, len - kEps, false))
                res = res + ((4.f * kPi * L.rad * L.rad) * wi * wo / (len * len)) * of(L.e);
        }
        f3 vres = mk(0.f, 0.f, 0.f);
        f3 vd = of(v.hp) - h;
        const float len = sqrtf(dot(vd, vd));
        vd = (1.f / len) * vd;
        float wo = dot(vd, of(v.nl));
        if (!(wo > 0.f)) {
            wo = -wo;
            const float wi = dot(vd, nl);
            if (wi > 0.f && !sc.occluded(h, vd, len - kEps, true)) vres = vres + (wi * wo) * of(v.rad);
        }
        vres = 1.f * vres;
        res = res + vres;
        return 0.5f * res;
    }

    // The camera ray of pixel (x, y): jittered with pass sid's randoms, or (+0, +0).
    eye_ray camera_ray(int x, int y, int W, bool jitter, unsigned sid) const {
        float u0 = 0.f, u1 = 0.f;
        if (jitter) {
            const unsigned kk = eye_rand_index((unsigned)(y * W + x), 0u, sid);
            u0 = rnd[kk];
            u1 = rnd[kk + 1];
        }
        return eye_camera_ray(cam, x, y, u0, u1);
    }

    // The vertices are bdpt_eye.h's; Scene::closest is the traversal between them.
    f3 sample(int x, int y, int W, unsigned sid, int vlp) const {
        eye_ray r = camera_ray(x, y, W, true, sid);
        f3 rad = mk(0.f, 0.f, 0.f), thr = mk(1.f, 1.f, 1.f);
        bool specular = true;
        const bdpt_lightpath& v = lp[vlp & (BDPT_LIGHT_POINTS - 1)];
        for (unsigned depth = 0; depth <= 6; ++depth) {
            const unsigned j = eye_rand_index((unsigned)(y * W + x), depth, sid);
            float t;
            unsigned id = 0;
            if (!sc.closest(r.o, r.d, &t, &id)) break;
            const bdpt_sphere& S = sc.s[id];
            const eye_vertex p = eye_vertex_at(r.o, r.d, t, of(S.p));
            if (sc.emissive[id]) {                                   // :651-661
                if (specular) rad = rad + thr * (fabsf(p.dp) * of(S.e));
                break;
            }
            r.o = p.hit;
            specular = S.refl != BDPT_DIFF;
            if (!specular) {                                         // :663-703
                const f3 nl = eye_nl(p.normal, p.dp);
                thr = thr * of(S.c);
                rad = rad + lights(p.hit, nl, j, v) * thr;
                r.d = cosine_dir(nl, rnd[j], rnd[j + 1]);
                continue;
            }
            eye_specular(S.refl == BDPT_SPEC, p.normal, p.dp, of(S.c), [&](float P) { return rnd[j + 2] < P; }, r.d,
                         thr);
        }
        return rad;
    }

    // The eye path of sample() up to its first non-specular vertex (include/bdpt.h bdpt_render_chain):
    // the same vertices, stopped at the first emitter, diffuse surface or miss.  pass: glass takes
    // pass sid's choice (rnd[j + 2] < P), else it transmits whenever refraction exists.
    struct Chain {
        int id = -1, first_id = -1, kind = BDPT_CHAIN_KIND_EXHAUSTED, bounces = 0;
        float t = 0.f, dp = 0.f;
        f3 pos = mk(0.f, 0.f, 0.f), nrm = mk(0.f, 0.f, 0.f), dir, thr = mk(1.f, 1.f, 1.f);
    };
    Chain chain(int x, int y, int W, bool jitter, unsigned sid, bool pass) const {
        eye_ray r = camera_ray(x, y, W, jitter, sid);
        Chain c;
        float len = 0.f;                                     // sums in locals, the result assembled after
        eye_vertex p = {c.pos, c.nrm, c.dp};                 // the loop: the shape that was timed
        for (unsigned depth = 0; depth <= 6; ++depth) {
            float t;
            unsigned id = 0;
            const bool hit = sc.closest(r.o, r.d, &t, &id);
            if (depth == 0) c.first_id = hit ? (int)id : -1;
            if (!hit) {
                c.kind = BDPT_CHAIN_KIND_MISS;
                break;
            }
            const bdpt_sphere& S = sc.s[id];
            len = len + t;
            p = eye_vertex_at(r.o, r.d, t, of(S.p));
            if (sc.emissive[id]) {                                   // :651, before the material
                c.kind = BDPT_CHAIN_KIND_EMITTER;
                c.id = (int)id;
                break;
            }
            if (S.refl == BDPT_DIFF) {
                c.kind = BDPT_CHAIN_KIND_DIFFUSE;
                c.id = (int)id;
                break;
            }
            c.bounces++;
            r.o = p.hit;
            eye_specular(S.refl == BDPT_SPEC, p.normal, p.dp, of(S.c), [&](float P) {
                return pass && rnd[eye_rand_index((unsigned)(y * W + x), depth, sid) + 2] < P;
            }, r.d, c.thr);
        }
        c.t = len;
        c.dir = r.d;
        if (c.kind == BDPT_CHAIN_KIND_DIFFUSE || c.kind == BDPT_CHAIN_KIND_EMITTER) {
            c.dp = p.dp; c.pos = p.hit; c.nrm = p.normal;
        }
        return c;
    }
};
}  // namespace

// npass x UpdateRendering (smallpt_cpu.c:265-297): each pixel of this context's shard renders its
// passes in order with the running mean of device.cu:774-787.  With a tile mask, only the pixels of
// the 32 x 8 tiles (anchored at (0, 0), row-major) whose byte is non-zero; the others are not touched.
void bdpt_cpu_path_passes(bdpt_cpu_ctx* c, const unsigned* sid, const int* vlp, int npass,
                          const unsigned char* tile_mask) {
    const PathTracer pt(c);
    const int W = c->W;
    const int tiles_x = (W + BDPT_NOISE_TW - 1) / BDPT_NOISE_TW;
    parallel_rows(0, c->H, c->threads, [&](int y) {
        if (c->nshards > 1 && (y / c->band_rows) % c->nshards != c->shard) return;
        const unsigned char* row = tile_mask ? tile_mask + (size_t)(y / BDPT_NOISE_TH) * tiles_x : nullptr;
        for (int x = 0; x < W; x++) {
            if (row && !row[x / BDPT_NOISE_TW]) {
                x = (x / BDPT_NOISE_TW + 1) * BDPT_NOISE_TW - 1;      // on to the next tile
                continue;
            }
            const size_t i = (size_t)y * W + x;
            bdpt_vec col = c->colors[i];
            unsigned cnt = c->counter[i];
            const unsigned cnt0 = cnt;
            for (int p = 0; p < npass && cnt < BDPT_COUNTER_CAP; p++, cnt++) {
                const f3 r = pt.sample(x, y, W, sid[p], vlp[p]);
                if (cnt == 0) {
                    col = {r.x, r.y, r.z};
                } else {
                    const float k1 = (float)cnt, k2 = 1.f / (k1 + 1.f);
                    col.x = (col.x * k1 + r.x) * k2;
                    col.y = (col.y * k1 + r.y) * k2;
                    col.z = (col.z * k1 + r.z) * k2;
                }
            }
            if (cnt == cnt0) continue;
            c->colors[i] = col;
            c->counter[i] = cnt;
            unsigned char* px = &c->pixels[4 * i];
            px[0] = (unsigned char)to_int8(col.x, c->thr);
            px[1] = (unsigned char)to_int8(col.y, c->thr);
            px[2] = (unsigned char)to_int8(col.z, c->thr);
            px[3] = 0;
        }
    });
}

// First-hit feature buffers (include/bdpt.h bdpt_render_aov): the first segment of the eye path of
// sample() on its own -- bdpt_eye.h's camera ray, IntersectDevice (:106-124) and bdpt_eye.h's vertex
// -- for the window's pixels, packed [h][w].  The caller has checked the window, the camera and
// (jitter) the table.
static void render_aov_cam(const bdpt_cpu_ctx* c, const bdpt_camera& cam, int x0, int y0, int w, int h, int jitter,
                           unsigned sid, const bdpt_aov_buffers* out) {
    const PathTracer pt(c, cam);
    const int W = c->W;
    parallel_rows(y0, y0 + h, c->threads, [&](int y) {
        for (int x = x0; x < x0 + w; x++) {
            const eye_ray r = pt.camera_ray(x, y, W, jitter != 0, sid);
            float t = 0.f;
            unsigned s = 0;
            int id = -1;
            eye_vertex p = {mk(0.f, 0.f, 0.f), mk(0.f, 0.f, 0.f), 0.f};      // a miss: +0 everywhere but dir
            if (pt.sc.closest(r.o, r.d, &t, &s)) {
                id = (int)s;
                p = eye_vertex_at(r.o, r.d, t, of(pt.sc.s[s].p));
            } else {
                t = 0.f;
            }
            const size_t k = (size_t)(y - y0) * w + (x - x0);
            if (out->id) out->id[k] = id;
            if (out->t) out->t[k] = t;
            if (out->dp) out->dp[k] = p.dp;
            if (out->position) out->position[k] = to_vec(p.hit);
            if (out->normal) out->normal[k] = to_vec(p.normal);
            if (out->dir) out->dir[k] = to_vec(r.d);
        }
    });
}

void bdpt_cpu_render_aov(const bdpt_cpu_ctx* c, int x0, int y0, int w, int h, int jitter, unsigned sid,
                         const bdpt_aov_buffers* out) {
    render_aov_cam(c, c->cam, x0, y0, w, h, jitter, sid, out);
}

// The eye path up to its first non-specular vertex (include/bdpt.h bdpt_render_chain) for the
// window's pixels, packed [h][w].  The caller has checked the window, the branch, the camera and
// (jitter) the table.
void bdpt_cpu_render_chain(const bdpt_cpu_ctx* c, int x0, int y0, int w, int h, int jitter, unsigned sid, int branch,
                           const bdpt_chain_buffers* out) {
    const PathTracer pt(c);
    const int W = c->W;
    parallel_rows(y0, y0 + h, c->threads, [&](int y) {
        for (int x = x0; x < x0 + w; x++) {
            const PathTracer::Chain r = pt.chain(x, y, W, jitter != 0, sid, branch == BDPT_CHAIN_PASS);
            const size_t k = (size_t)(y - y0) * w + (x - x0);
            if (out->id) out->id[k] = r.id;
            if (out->first_id) out->first_id[k] = r.first_id;
            if (out->kind) out->kind[k] = r.kind;
            if (out->bounces) out->bounces[k] = r.bounces;
            if (out->t) out->t[k] = r.t;
            if (out->dp) out->dp[k] = r.dp;
            if (out->position) out->position[k] = {r.pos.x, r.pos.y, r.pos.z};
            if (out->normal) out->normal[k] = {r.nrm.x, r.nrm.y, r.nrm.z};
            if (out->dir) out->dir[k] = {r.dir.x, r.dir.y, r.dir.z};
            if (out->throughput) out->throughput[k] = {r.thr.x, r.thr.y, r.thr.z};
        }
    });
}

namespace {
// The unjittered whole-frame first hit under `cam`: the ids and the planes asked for.
enum { kHitPos = 1, kHitT = 2, kHitNrm = 4 };
struct FirstHit {
    std::vector<int> id;
    std::vector<float> t;
    std::vector<bdpt_vec> pos, nrm;
    FirstHit(const bdpt_cpu_ctx* c, const bdpt_camera& cam, int planes) {
        const size_t np = (size_t)c->W * c->H;
        bdpt_aov_buffers g;
        memset(&g, 0, sizeof g);
        id.resize(np);
        g.id = id.data();
        if (planes & kHitPos) { pos.resize(np); g.position = pos.data(); }
        if (planes & kHitT) { t.resize(np); g.t = t.data(); }
        if (planes & kHitNrm) { nrm.resize(np); g.normal = nrm.data(); }
        render_aov_cam(c, cam, 0, 0, c->W, c->H, 0, 0u, &g);
    }
    // the ids as the filters' guide ids: an ineligible pixel gets -1
    void to_guide_ids(const bdpt_cpu_ctx* c, int materials) {
        for (int& g : id) g = guide_id(g, materials == BDPT_DENOISE_ALL, c->scene.s.data());
    }
    // The denoisers' guides by `materials`: the first hit's ids made guide ids, or
    // (BDPT_DENOISE_THROUGH, include/bdpt.h) the key and end normal of the unjittered TRANSMIT chain.
    struct Guides {};
    FirstHit(const bdpt_cpu_ctx* c, int materials, Guides) {
        if (materials != BDPT_DENOISE_THROUGH) {
            *this = FirstHit(c, c->cam, kHitNrm);
            to_guide_ids(c, materials);
            return;
        }
        const size_t np = (size_t)c->W * c->H;
        std::vector<int> kind(np), bounces(np), first(np);
        id.resize(np);
        nrm.resize(np);
        bdpt_chain_buffers g;
        memset(&g, 0, sizeof g);
        g.id = id.data(); g.first_id = first.data(); g.kind = kind.data(); g.bounces = bounces.data();
        g.normal = nrm.data();
        bdpt_cpu_render_chain(c, 0, 0, c->W, c->H, 0, 0u, BDPT_CHAIN_TRANSMIT, &g);
        const int n = (int)c->scene.n;
        for (size_t i = 0; i < np; i++)
            id[i] = through_key(kind[i] == BDPT_CHAIN_KIND_DIFFUSE, n, bounces[i], first[i], id[i]);
    }
};

// The levels of the three a-trous filters (bdpt_filter.h lv_tap / lv_finish; MODE as the kernels'
// kLvPlain / kLvCounts / kLvNoise), ping-pong from `ping` and, in the modes that carry a count or a
// variance, `aping`; the result is left there.  Level l has step 2^l and isc0 * 4^l; kk is c2 or
// s2.  A tap counts when it is inside the frame and shows the centre's sphere; an ineligible pixel
// is copied through.  Threaded over rows per level.  (The tap loops are written out here and in the
// prefilter: as a callback of a shared loop they are slower.)
template <int MODE>
void atrous_levels(const bdpt_cpu_ctx* c, const FirstHit& g, int levels, int normal_power, float sigma_color,
                   float kk, std::vector<bdpt_vec>& ping, std::vector<float>& aping) {
    const int W = c->W, H = c->H;
    std::vector<bdpt_vec> pong(ping.size());
    std::vector<float> apong(aping.size());
    const float isc0 = 1.0f / (sigma_color * sigma_color);
    for (int l = 0; l < levels; l++) {
        const int step = 1 << l;
        const float isc = isc0 * (float)(1 << (2 * l));
        const bdpt_vec* cur = ping.data();
        const float* acur = aping.data();
        bdpt_vec* out = pong.data();
        float* aout = apong.data();
        parallel_rows(0, H, c->threads, [&](int y) {
            for (int x = 0; x < W; x++) {
                const size_t i = (size_t)y * W + x;
                const f3 c_p = of(cur[i]);
                float a_p = 0.f;
                if constexpr (MODE != kLvPlain) a_p = acur[i];
                f3 o = c_p;
                float a = a_p;
                if (g.id[i] >= 0) {
                    const f3 n_p = of(g.nrm[i]);
                    float su = 0.f, sw = 0.f;
                    f3 sc = mk(0.f, 0.f, 0.f);
                    bool used = false;
                    for (int j = 0; j < 5; j++) {
                        const int qy = y + (j - 2) * step;
                        if (qy < 0 || qy >= H) continue;
                        for (int t = 0; t < 5; t++) {
                            const int qx = x + (t - 2) * step;
                            if (qx < 0 || qx >= W) continue;
                            const size_t q = (size_t)qy * W + qx;
                            if (g.id[q] != g.id[i]) continue;
                            float a_q = 0.f;
                            if constexpr (MODE != kLvPlain) a_q = acur[q];
                            lv_tap<MODE>(b3_weight(j, t), normal_power, isc, kk, n_p, c_p, a_p, of(g.nrm[q]),
                                         of(cur[q]), a_q, su, sw, sc, used);
                        }
                    }
                    o = lv_finish<MODE>(used, c_p, a_p, su, sw, sc, a);
                }
                out[i] = to_vec(o);
                if constexpr (MODE != kLvPlain) aout[i] = a;
            }
        });
        ping.swap(pong);
        aping.swap(apong);
    }
}

// a service's frame to the caller's buffers, each optional
void write_frame(const bdpt_cpu_ctx* c, const std::vector<bdpt_vec>& col, bdpt_vec* colors_out,
                 unsigned char* rgba_out) {
    if (colors_out) memcpy(colors_out, col.data(), sizeof(bdpt_vec) * col.size());
    if (rgba_out) to_rgba(c->thr, col.data(), col.size(), rgba_out);
}
void write_plane(const std::vector<float>& a, float* out) {
    if (out) memcpy(out, a.data(), sizeof(float) * a.size());
}
}  // namespace

// Edge-avoiding wavelet denoiser (include/bdpt.h bdpt_denoise).  Guides: id and
// normal of the unjittered first hit; then the plain levels.  The caller has checked the parameters
// and the camera; the context's own state is only read.
void bdpt_cpu_denoise(const bdpt_cpu_ctx* c, const bdpt_denoise_params* p, bdpt_vec* colors_out,
                      unsigned char* rgba_out) {
    const FirstHit g(c, p->materials, FirstHit::Guides{});
    std::vector<bdpt_vec> ping(c->colors);
    std::vector<float> none;
    atrous_levels<kLvPlain>(c, g, p->levels, p->normal_power, p->sigma_color, 0.f, ping, none);
    write_frame(c, ping, colors_out, rgba_out);
}

// Temporal reprojection (include/bdpt.h bdpt_reproject): the current camera's
// unjittered first hit, its point projected into the history's camera, four validated bilinear
// taps, the blend by sample count -- bdpt_filter.h's rp_project, rp_tap, rp_history and rp_blend.
// The state of a history taken under s0[n0] against the spheres s[n] (include/bdpt.h
// bdpt_history_motion: the followable rule and the offsets), host code shared by both backends.
// delta (n entries, may be nullptr) is written in the states SAME and MOVED only.
int bdpt_history_state(bool stored, const bdpt_sphere* s0, size_t n0, const bdpt_sphere* s, size_t n, bdpt_vec* delta) {
    if (!stored) return BDPT_HISTORY_NONE;
    if (n0 != n) return BDPT_HISTORY_UNUSABLE;
    if (n == 0 || memcmp(s0, s, sizeof(bdpt_sphere) * n) == 0) {
        if (delta)
            for (size_t k = 0; k < n; k++) delta[k] = {0.f, 0.f, 0.f};
        return BDPT_HISTORY_SAME;
    }
    for (size_t k = 0; k < n; k++) {
        const bdpt_sphere &a = s0[k], &b = s[k];
        if (memcmp(&a.rad, &b.rad, sizeof a.rad) || memcmp(&a.e, &b.e, sizeof a.e) || memcmp(&a.c, &b.c, sizeof a.c) ||
            memcmp(&a.refl, &b.refl, sizeof a.refl))
            return BDPT_HISTORY_UNUSABLE;
        const bool emits = !(b.e.x == 0.f && b.e.y == 0.f && b.e.z == 0.f);
        if (emits && memcmp(&a.p, &b.p, sizeof a.p)) return BDPT_HISTORY_UNUSABLE;
    }
    if (delta)
        for (size_t k = 0; k < n; k++) {
            const bdpt_vec &a = s0[k].p, &b = s[k].p;
            delta[k] = {b.x == a.x ? 0.f : b.x - a.x, b.y == a.y ? 0.f : b.y - a.y, b.z == a.z ? 0.f : b.z - a.z};
        }
    return BDPT_HISTORY_MOVED;
}

void bdpt_cpu_history_follow(bdpt_cpu_ctx* c, int on) { c->follow = on != 0; }
int bdpt_cpu_history_motion(const bdpt_cpu_ctx* c, bdpt_vec* delta) {
    return bdpt_history_state(c->has_hist, c->hsph.data(), c->hsph.size(), c->scene.s.data(), c->scene.s.size(), delta);
}
bool bdpt_cpu_history_present(const bdpt_cpu_ctx* c) {
    const int state = bdpt_cpu_history_motion(c, nullptr);
    return state == BDPT_HISTORY_SAME || (c->follow && state == BDPT_HISTORY_MOVED);
}
bool bdpt_cpu_history_stored(const bdpt_cpu_ctx* c, bdpt_camera* cam) {
    if (c->has_hist && cam) *cam = c->hcam;
    return c->has_hist;
}
void bdpt_cpu_history_clear(bdpt_cpu_ctx* c) { c->has_hist = false; }
void bdpt_cpu_history_read(const bdpt_cpu_ctx* c, bdpt_vec* colors, float* weight) {
    if (colors) memcpy(colors, c->hc.data(), sizeof(bdpt_vec) * c->hc.size());
    if (weight) memcpy(weight, c->hm.data(), sizeof(float) * c->hm.size());
}

namespace {
// (out, weight_out) of the whole frame from the history present, if any
void reproject_frame(const bdpt_cpu_ctx* c, const bdpt_reproject_params* p, const FirstHit& f,
                     std::vector<bdpt_vec>& out, std::vector<float>& wout) {
    const int W = c->W, H = c->H;
    // "follow": the offsets of a history whose spheres have moved (empty: P stands as it is)
    std::vector<bdpt_vec> delta(c->follow ? c->scene.s.size() : 0);
    const int state = bdpt_cpu_history_motion(c, delta.empty() ? nullptr : delta.data());
    const bool present = state == BDPT_HISTORY_SAME || (c->follow && state == BDPT_HISTORY_MOVED);
    if (state != BDPT_HISTORY_MOVED) delta.clear();
    const bool all_materials = p->materials == BDPT_DENOISE_ALL;
    const eye_camera c0 = eye_camera_terms(c->hcam, W, H);
    const f3 ux = c0.ux, uy = c0.uy, ud = c0.ud, o = c0.orig;
    const float hw = (float)c0.half_w, hh = (float)c0.half_h;
    const float sx = 1.f / c0.inv_w, sy = 1.f / c0.inv_h;
    parallel_rows(0, H, c->threads, [&](int y) {
        for (int x = 0; x < W; x++) {
            const size_t i = (size_t)y * W + x;
            const int id1 = f.id[i];
            float m = 0.f;
            f3 h = mk(0.f, 0.f, 0.f);
            if (present && guide_id(id1, all_materials, c->scene.s.data()) >= 0) {
                const f3 N = of(f.nrm[i]);
                const f3 P = delta.empty() ? of(f.pos[i]) : rp_follow(of(f.pos[i]), of(delta[id1]));
                float fx, fy;
                if (rp_project(P, o, ux, uy, ud, hw, hh, sx, sy, W, H, fx, fy)) {
                    const float xf = floorf(fx), yf = floorf(fy);
                    const float wx = fx - xf, wy = fy - yf;
                    const int qx0 = (int)xf, qy0 = (int)yf;       // -1 .. W-1, -1 .. H-1
                    const float lim = p->plane_tol * f.t[i];
                    float sw = 0.f, sm = 0.f;
                    f3 sc = mk(0.f, 0.f, 0.f);
                    bool used = false;
                    for (int k = 0; k < 4; k++) {
                        const int qx = qx0 + (k & 1), qy = qy0 + (k >> 1);
                        const bool in = qx >= 0 && qx < W && qy >= 0 && qy < H;
                        const size_t q = in ? (size_t)qy * W + qx : i;   // outside: the pixel's own, not used
                        rp_tap(k, wx, wy, in, c->gid[q], of(c->gpos[q]), of(c->hc[q]), c->hm[q], id1, P, N, lim,
                               p->max_history, sw, sm, sc, used);
                    }
                    rp_history(used, sw, sm, sc, h, m);
                }
            }
            out[i] = to_vec(rp_blend(of(c->colors[i]), (float)c->counter[i], h, m, wout[i]));
        }
    });
}
}  // namespace

void bdpt_cpu_reproject(const bdpt_cpu_ctx* c, const bdpt_reproject_params* p, bdpt_vec* colors_out,
                        float* weight_out, unsigned char* rgba_out) {
    const size_t np = (size_t)c->W * c->H;
    const FirstHit f(c, c->cam, kHitPos | kHitT | kHitNrm);
    std::vector<bdpt_vec> out(np);
    std::vector<float> w(np);
    reproject_frame(c, p, f, out, w);
    write_frame(c, out, colors_out, rgba_out);
    write_plane(w, weight_out);
}

// Count-weighted denoising of the reprojected preview (include/bdpt.h bdpt_preview_denoise;
// DESIGN.md 4f).  The input is reproject_frame's (out, tot); the guides are the first hit the
// reprojection has just used; a record's count is clamped when the record is written; then the
// levels with counts.  levels == 0 is the reprojection itself.  The caller has checked the parameters.
void bdpt_cpu_preview_denoise(const bdpt_cpu_ctx* c, const bdpt_preview_params* p, bdpt_vec* colors_out,
                              float* weight_out, unsigned char* rgba_out) {
    const size_t np = (size_t)c->W * c->H;
    FirstHit f(c, c->cam, kHitPos | kHitT | kHitNrm);
    std::vector<bdpt_vec> ping(np);
    std::vector<float> aping(np);
    reproject_frame(c, &p->rp, f, ping, aping);
    if (p->levels > 0) {
        f.to_guide_ids(c, p->rp.materials);
        for (float& a : aping) a = clampc(a);
        atrous_levels<kLvCounts>(c, f, p->levels, p->normal_power, p->sigma_color, 2.f / p->count_ref, ping, aping);
    }
    write_frame(c, ping, colors_out, rgba_out);
    write_plane(aping, weight_out);
}

// The new history is formed in buffers of its own while the old one is read, then swapped in; its
// guides are the first hit the reprojection has just used (the current camera becomes C0).
void bdpt_cpu_history_capture(bdpt_cpu_ctx* c, const bdpt_reproject_params* p) {
    const size_t np = (size_t)c->W * c->H;
    FirstHit f(c, c->cam, kHitPos | kHitT | kHitNrm);
    std::vector<bdpt_vec> out(np);
    std::vector<float> w(np);
    reproject_frame(c, p, f, out, w);
    c->hc.swap(out);
    c->hm.swap(w);
    c->gid.swap(f.id);
    c->gpos.swap(f.pos);
    c->hcam = c->cam;
    c->hsph = c->scene.s;
    c->has_hist = true;
}

void bdpt_cpu_history_write(bdpt_cpu_ctx* c, const bdpt_camera* cam, const bdpt_vec* colors, const float* weight) {
    const size_t np = (size_t)c->W * c->H;
    FirstHit f(c, *cam, kHitPos);
    c->hc.assign(colors, colors + np);
    c->hm.assign(weight, weight + np);
    c->gid.swap(f.id);
    c->gpos.swap(f.pos);
    c->hcam = *cam;
    c->hsph = c->scene.s;
    c->has_hist = true;
}

bool bdpt_cpu_rand_ready(const bdpt_cpu_ctx* c) { return c->rand_ready; }
bool bdpt_cpu_camera_set(const bdpt_cpu_ctx* c) { return c->cam_set; }

void bdpt_cpu_read_radiance(const bdpt_cpu_ctx* c, bdpt_vec* colors, unsigned* counter) {
    if (colors) memcpy(colors, c->colors.data(), sizeof(bdpt_vec) * c->colors.size());
    if (counter) memcpy(counter, c->counter.data(), sizeof(unsigned) * c->counter.size());
}
void bdpt_cpu_read_pixels(const bdpt_cpu_ctx* c, unsigned char* rgba) { memcpy(rgba, c->pixels.data(), c->pixels.size()); }
void bdpt_cpu_read_rand(const bdpt_cpu_ctx* c, float* t) { memcpy(t, c->rnd.data(), sizeof(float) * kRandN); }
void bdpt_cpu_write_rand(bdpt_cpu_ctx* c, const float* t) {
    c->rnd.assign(t, t + kRandN);
    c->rand_ready = true;
}
void bdpt_cpu_read_lightpaths(const bdpt_cpu_ctx* c, bdpt_lightpath* lp) {
    memcpy(lp, c->lp.data(), sizeof(bdpt_lightpath) * BDPT_LIGHT_POINTS);
}
void bdpt_cpu_write_lightpaths(bdpt_cpu_ctx* c, const bdpt_lightpath* lp) {
    memcpy(c->lp.data(), lp, sizeof(bdpt_lightpath) * BDPT_LIGHT_POINTS);
}
void bdpt_cpu_update_pixels(bdpt_cpu_ctx* c) {
    to_rgba(c->thr, c->colors.data(), c->colors.size(), c->pixels.data());
}
void bdpt_cpu_write_radiance(bdpt_cpu_ctx* c, const bdpt_vec* colors, const unsigned* counter) {
    memcpy(c->colors.data(), colors, sizeof(bdpt_vec) * c->colors.size());
    memcpy(c->counter.data(), counter, sizeof(unsigned) * c->counter.size());
    bdpt_cpu_update_pixels(c);
    bdpt_cpu_noise_clear(c);
}

// Per-tile noise estimate (include/bdpt.h bdpt_noise_estimate): the mark rules and
// the per-pixel error are bdpt_filter.h's; the tile's sum is the definition's adjacent-pair tree
// over its 256 slots, which the HIP kernel's wave butterfly is checked against.
bool bdpt_cpu_noise_stored(const bdpt_cpu_ctx* c) { return !c->mark.empty(); }
void bdpt_cpu_noise_clear(bdpt_cpu_ctx* c) {
    for (auto& m : c->mark) m.n = 0u;                     // nothing while no mark was ever stored
}
void bdpt_cpu_noise_write_mark(bdpt_cpu_ctx* c, const bdpt_vec* colors, const unsigned* counter) {
    c->mark.resize(c->colors.size());
    for (size_t i = 0; i < c->mark.size(); i++) c->mark[i] = {colors[i], counter[i]};
}
void bdpt_cpu_noise_mark(bdpt_cpu_ctx* c) { bdpt_cpu_noise_write_mark(c, c->colors.data(), c->counter.data()); }
void bdpt_cpu_noise_read_mark(const bdpt_cpu_ctx* c, bdpt_vec* colors, unsigned* counter) {
    for (size_t i = 0; i < c->mark.size(); i++) {
        if (colors) colors[i] = c->mark[i].c;
        if (counter) counter[i] = c->mark[i].n;
    }
}

void bdpt_cpu_noise_estimate(bdpt_cpu_ctx* c, const bdpt_noise_params* p, float* error_out, float* tile_sum,
                             float* tile_error, unsigned* tile_valid, unsigned* tile_pending) {
    const int W = c->W, H = c->H;
    const int tx = (W + BDPT_NOISE_TW - 1) / BDPT_NOISE_TW, ty = (H + BDPT_NOISE_TH - 1) / BDPT_NOISE_TH;
    if (p->remark && c->mark.empty()) c->mark.assign((size_t)W * H, {bdpt_vec{0.f, 0.f, 0.f}, 0u});
    const bool stored = !c->mark.empty();
    c->last_pending.assign((size_t)tx * ty, 0u);
    for (int by = 0; by < ty; by++)
        for (int bx = 0; bx < tx; bx++) {
            float v[BDPT_NOISE_TW * BDPT_NOISE_TH];
            unsigned valid = 0, pending = 0;
            for (int k = 0; k < BDPT_NOISE_TW * BDPT_NOISE_TH; k++) {
                const int x = bx * BDPT_NOISE_TW + k % BDPT_NOISE_TW, y = by * BDPT_NOISE_TH + k / BDPT_NOISE_TW;
                v[k] = 0.f;
                if (x >= W || y >= H) continue;
                const size_t i = (size_t)y * W + x;
                const bdpt_vec B = c->colors[i];
                const unsigned cnt = c->counter[i], mn = stored ? c->mark[i].n : 0u;
                float e = -1.0f;
                if (mark_valid(cnt, mn)) {
                    e = pixel_error(of(B), of(c->mark[i].c), cnt, mn, p->dark);
                    v[k] = e;
                    valid++;
                } else if (mark_growing(cnt)) {
                    pending++;
                }
                if (error_out) error_out[i] = e;
                if (p->remark && mark_take(cnt, mn)) c->mark[i] = {B, cnt};
            }
            for (int m = BDPT_NOISE_TW * BDPT_NOISE_TH; m > 1; m /= 2)   // adjacent pairs, eight rounds
                for (int k = 0; k < m / 2; k++) v[k] = v[2 * k] + v[2 * k + 1];
            const int t = by * tx + bx;
            if (tile_sum) tile_sum[t] = v[0];
            if (tile_error) tile_error[t] = valid ? v[0] / (float)valid : 0.f;
            if (tile_valid) tile_valid[t] = valid;
            if (tile_pending) tile_pending[t] = pending;
            c->last_pending[t] = pending;
        }
}
bool bdpt_cpu_noise_tile_pending(const bdpt_cpu_ctx* c, unsigned* tile_pending) {
    if (c->last_pending.empty()) return false;
    memcpy(tile_pending, c->last_pending.data(), sizeof(unsigned) * c->last_pending.size());
    return true;
}

// Noise-guided denoiser (include/bdpt.h bdpt_denoise_noise): the raw variance from
// the mark, its 5x5 prefilter, then the denoiser's levels with the colour stop scaled by the two
// pixels' variances and the variance carried along.  Threaded over rows.
void bdpt_cpu_denoise_noise(const bdpt_cpu_ctx* c, const bdpt_denoise_noise_params* p, bdpt_vec* colors_out,
                            unsigned char* rgba_out, float* variance_out) {
    const int W = c->W, H = c->H;
    const size_t np = (size_t)W * H;
    const FirstHit g(c, p->materials, FirstHit::Guides{});
    const bool stored = !c->mark.empty();
    std::vector<float> v0(np, -1.0f), var(np);
    for (size_t i = 0; i < np; i++) {                     // the raw variance
        const unsigned cnt = c->counter[i], mn = stored ? c->mark[i].n : 0u;
        if (mark_valid(cnt, mn)) v0[i] = raw_variance(of(c->colors[i]), of(c->mark[i].c), cnt, mn);
    }
    parallel_rows(0, H, c->threads, [&](int y) {          // the prefilter
        for (int x = 0; x < W; x++) {
            const size_t i = (size_t)y * W + x;
            var[i] = v0[i];
            if (g.id[i] < 0) continue;
            float sv = 0.f, sh = 0.f;
            bool used = false;
            for (int j = 0; j < 5; j++) {
                const int qy = y + (j - 2);
                if (qy < 0 || qy >= H) continue;
                for (int t = 0; t < 5; t++) {
                    const int qx = x + (t - 2);
                    if (qx < 0 || qx >= W) continue;
                    const size_t q = (size_t)qy * W + qx;
                    pf_tap(b3_weight(j, t), g.id[q] == g.id[i], v0[q], sv, sh, used);
                }
            }
            var[i] = pf_finish(used, sv, sh);
        }
    });
    std::vector<bdpt_vec> ping(c->colors);
    atrous_levels<kLvNoise>(c, g, p->levels, p->normal_power, p->sigma_color, p->noise_sigma * p->noise_sigma, ping,
                            var);
    write_frame(c, ping, colors_out, rgba_out);
    write_plane(var, variance_out);
}

// The frame's summary from the tile arrays in row-major order: the one statement of it, shared by
// both backends (and the sanitizer build's context layer).
void bdpt_noise_summarize(const float* tile_sum, const float* tile_error, const unsigned* tile_valid,
                          const unsigned* tile_pending, int tiles_x, int tiles_y, float threshold,
                          bdpt_noise_summary* out) {
    bdpt_noise_summary s;
    memset(&s, 0, sizeof s);
    s.tiles_x = tiles_x;
    s.tiles_y = tiles_y;
    double sum = 0.;
    float m = 0.f;
    for (int t = 0; t < tiles_x * tiles_y; t++) {
        s.valid_pixels += tile_valid[t];
        s.pending_pixels += tile_pending[t];
        s.valid_tiles += tile_valid[t] > 0u;
        sum += (double)tile_sum[t];
        if (tile_error[t] > m) m = tile_error[t];
        s.tiles_over += tile_error[t] > threshold;
    }
    s.mean = s.valid_pixels ? sum / (double)s.valid_pixels : 0.;
    s.max_tile = m;
    *out = s;
}
