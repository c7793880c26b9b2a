// bdpt_frame.cpp -- the frame services of the C-ABI (include/bdpt.h): first-hit feature buffers and
// picking, the denoiser, the history and its reprojection, the denoised preview and the noise
// estimate, over the kernels of bdpt_frame_kernels.h and bdpt_aov_kernel (bdpt_kernels.hip).
//
// Every service runs on the context's stream after the last fold (bdpt_host::join_fold), reads
// what the path passes left and touches nothing of their state: not the accumulation, not the
// timing ring, not the stream choice.  What they share is written once, in the scaffold below: the
// per-service clock, the first-hit launch, the buffers, the level loop, the reprojection launch and
// the read-back.  No reference counterpart.
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <chrono>
#include <vector>

#include "bdpt_ctx.h"

using namespace bdpt_host;

extern "C" __global__ void bdpt_aov_kernel(bdpt_path_args, bdpt_aov_args);
extern "C" __global__ void bdpt_chain_kernel(bdpt_path_args, bdpt_chain_args);
extern "C" __global__ void bdpt_denoise_pack_kernel(const int*, const bdpt_dev_vec*, const bdpt_dev_vec*,
                                                    const bdpt_dev_sphere*, int, float4*, float4*, int);
extern "C" const void* bdpt_denoise_level_table[2][7];   // [LDS staging][normal_power]
extern "C" __global__ void bdpt_history_pack_kernel(const int*, const bdpt_dev_vec*, const bdpt_dev_vec*,
                                                    const float*, float4*, float4*, int);
extern "C" __global__ void bdpt_reproject_kernel(bdpt_reproject_args);
extern "C" const void* bdpt_preview_level_table[2][7];   // [LDS staging][normal_power]
extern "C" __global__ void bdpt_noise_mark_kernel(const bdpt_dev_vec*, const unsigned*, uint4*, int);
extern "C" __global__ void bdpt_noise_kernel(bdpt_noise_args);
extern "C" __global__ void bdpt_dnoise_pack_kernel(const int*, const bdpt_dev_vec*, const bdpt_dev_vec*, const unsigned*,
                                                   const uint4*, int, const bdpt_dev_sphere*, int, float4*, float4*, int);
extern "C" __global__ void bdpt_dnoise_prefilter_kernel(const float4*, const float4*, float4*, int, int);
extern "C" const void* bdpt_dnoise_level_table[2][7];    // [LDS staging][normal_power]
static_assert(BDPT_NOISE_BTW == BDPT_NOISE_TW && BDPT_NOISE_BTH == BDPT_NOISE_TH, "the kernel's tile is the ABI's");

// ---- the shared scaffold ---------------------------------------------------------------------

static unsigned cdiv(size_t n, int b) { return (unsigned)((n + (size_t)b - 1) / (size_t)b); }
static dim3 tile_grid(int w, int h, int btw, int bth) { return dim3(cdiv((size_t)w, btw), cdiv((size_t)h, bth), 1); }
static dim3 lane_grid(size_t np) { return dim3(cdiv(np, 256)); }   // one lane per pixel, 256-thread workgroups

// The clock of service s (kSvc*).  GPU: svc_begin / svc_end record the events around the launches
// between them, so no allocation and no read-back belongs there.  CPU backend: svc_cpu times the call.
static int svc_begin(bdpt_ctx* c, int s) {
    bdpt_svc_clock& k = c->svc[s];
    for (hipEvent_t& e : k.ev)
        if (!e) HIPCHK(c, hipEventCreate(&e));
    HIPCHK(c, hipEventRecord(k.ev[0], c->stream));
    return BDPT_OK;
}
static int svc_end(bdpt_ctx* c, int s) {
    HIPCHK(c, hipEventRecord(c->svc[s].ev[1], c->stream));
    c->svc[s].ran = true;
    return BDPT_OK;
}
template <class F>
static void svc_cpu(bdpt_ctx* c, int s, F call) {
    const auto t0 = std::chrono::steady_clock::now();
    call();
    c->svc[s].cpu_ms = (float)std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    c->svc[s].ran = true;
}
// bdpt_last_*_ms; `none` is the message of a service that has not run
static int svc_last_ms(bdpt_ctx* c, int s, float* ms, const char* none) {
    if (!c || !ms) return BDPT_EINVAL;
    const bdpt_svc_clock& k = c->svc[s];
    if (!k.ran) return fail(c, BDPT_ESTATE, "%s", none);
    if (c->cpu) {
        *ms = k.cpu_ms;
        return BDPT_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipEventSynchronize(k.ev[1]));
    HIPCHK(c, hipEventElapsedTime(ms, k.ev[0], k.ev[1]));
    return BDPT_OK;
}

// Capacity of d_aov, bdpt_aov_kernel's arguments and its launch on the context's stream (`timed`:
// inside the feature buffers' clock, which then covers the kernel alone); the caller has checked
// the window, the camera and the table.  *vout holds the output planes on return.  The denoiser,
// the reprojection and the preview take their guides from these planes (aov_frame).
// A context-owned plane buffer of `words` words per pixel, grown to np pixels on demand.
static int planes_reserve(bdpt_ctx* c, const char* who, float** buf, size_t* cap, size_t np, size_t words) {
    if (np <= *cap) return BDPT_OK;
    HIPCHK(c, hipStreamSynchronize(c->stream));               // an earlier call's copies are done anyway
    if (*buf) HIPCHK(c, hipFree(*buf));
    *buf = nullptr;
    *cap = 0;
    if (hipMalloc(buf, words * sizeof(float) * np) != hipSuccess) {
        *buf = nullptr;
        return fail(c, BDPT_ENOMEM, "%s: output planes (%zu B)", who, words * sizeof(float) * np);
    }
    *cap = np;
    return BDPT_OK;
}
// The scene, camera and traversal arguments bdpt_aov_kernel and bdpt_chain_kernel share; returns
// whether the BVH is traversed.
static bool ray_args(bdpt_ctx* c, const bdpt_camera& cam, bdpt_path_args& a) {
    memset(&a, 0, sizeof(a));
    a.n = (unsigned)c->spheres.size();
    a.geom = c->d_geom;
    a.rnd = c->d_rand;
    camera_args(c, cam, a);
    const bool bvh = c->has_bvh && c->traversal != BDPT_TRAVERSE_BRUTE;
    if (bvh) bvh_args(c, a);
    return bvh;
}
static int aov_launch(bdpt_ctx* c, const bdpt_camera& cam, int x0, int y0, int w, int h, int jitter, unsigned sid,
                      bool timed, bdpt_aov_args* vout) {
    const size_t np = (size_t)w * (size_t)h;
    if (int rc = planes_reserve(c, "bdpt_render_aov", &c->d_aov, &c->aov_cap, np, 12)) return rc;
    bdpt_path_args a;
    const bool bvh = ray_args(c, cam, a);
    bdpt_aov_args v;
    memset(&v, 0, sizeof(v));
    v.x0 = x0; v.y0 = y0; v.w = w; v.h = h;
    v.jitter = jitter != 0;
    v.sid = sid;
    v.bvh = bvh;
    v.rows = !bvh;
    if (const char* e = getenv("BDPT_AOV_TILE")) {            // experiments: 8 = 8x8 wave tiles, 64 = rows
        if (atoi(e) == 8) v.rows = 0;
        if (atoi(e) == 64) v.rows = 1;
    }
    float* base = c->d_aov;
    v.id = (int*)base;
    v.t = base + c->aov_cap;
    v.dp = base + 2 * c->aov_cap;
    v.position = (bdpt_dev_vec*)(base + 3 * c->aov_cap);
    v.normal = (bdpt_dev_vec*)(base + 6 * c->aov_cap);
    v.dir = (bdpt_dev_vec*)(base + 9 * c->aov_cap);
    const dim3 grid = v.rows ? tile_grid(w, h, BDPT_AOV_ROW_BTW, BDPT_AOV_ROW_BTH)
                             : tile_grid(w, h, BDPT_AOV_BVH_BTW, BDPT_AOV_BVH_BTH);
    if (timed)
        if (int rc = svc_begin(c, kSvcAov)) return rc;
    hipLaunchKernelGGL(bdpt_aov_kernel, grid, dim3(256), 0, c->stream, a, v);
    HIPCHK(c, hipGetLastError());
    if (timed)
        if (int rc = svc_end(c, kSvcAov)) return rc;
    *vout = v;
    return BDPT_OK;
}
// the unjittered first hit of the whole frame under `cam`
static int aov_frame(bdpt_ctx* c, const bdpt_camera& cam, bdpt_aov_args* av) {
    return aov_launch(c, cam, 0, 0, c->W, c->H, 0, 0u, false, av);
}

// bdpt_chain_kernel's arguments and its launch on the context's stream, as aov_launch's.  keys ==
// false: the ten planes of bdpt_render_chain in d_chain (`timed`: inside the chain's clock).  keys:
// the denoisers' "through" guides of the whole frame -- the guide key and the end normal, written
// where aov_frame leaves the first hit's id and normal (d_aov), so the pack kernels read them there.
// Wave tile: rows for the brute scan and 8 x 8 for the BVH, as measured;
// BDPT_CHAIN_TILE = 8 / 64 overrides it for experiments.
static int chain_launch(bdpt_ctx* c, int x0, int y0, int w, int h, int jitter, unsigned sid, int branch, bool keys,
                        bool timed, bdpt_chain_args* vout) {
    const size_t np = (size_t)w * (size_t)h;
    if (keys) {
        if (int rc = planes_reserve(c, "bdpt_denoise", &c->d_aov, &c->aov_cap, np, 12)) return rc;
    } else {
        if (int rc = planes_reserve(c, "bdpt_render_chain", &c->d_chain, &c->chain_cap, np, BDPT_CHAIN_WORDS)) return rc;
    }
    bdpt_path_args a;
    const bool bvh = ray_args(c, c->cam, a);
    bdpt_chain_args v;
    memset(&v, 0, sizeof(v));
    v.x0 = x0; v.y0 = y0; v.w = w; v.h = h;
    v.jitter = jitter != 0;
    v.sid = sid;
    v.bvh = bvh;
    v.rows = !bvh;
    if (const char* e = getenv("BDPT_CHAIN_TILE")) {
        if (atoi(e) == 8) v.rows = 0;
        if (atoi(e) == 64) v.rows = 1;
    }
    v.pass = branch == BDPT_CHAIN_PASS;
    v.sph = c->d_sph;
    if (keys) {
        v.key_n = (int)c->spheres.size();
        v.id = (int*)c->d_aov;
        v.normal = (bdpt_dev_vec*)(c->d_aov + 6 * c->aov_cap);
    } else {
        float* base = c->d_chain;
        const size_t cap = c->chain_cap;
        v.id = (int*)base;
        v.first_id = (int*)(base + cap);
        v.kind = (int*)(base + 2 * cap);
        v.bounces = (int*)(base + 3 * cap);
        v.t = base + 4 * cap;
        v.dp = base + 5 * cap;
        v.position = (bdpt_dev_vec*)(base + 6 * cap);
        v.normal = (bdpt_dev_vec*)(base + 9 * cap);
        v.dir = (bdpt_dev_vec*)(base + 12 * cap);
        v.throughput = (bdpt_dev_vec*)(base + 15 * cap);
    }
    const dim3 grid = v.rows ? tile_grid(w, h, BDPT_AOV_ROW_BTW, BDPT_AOV_ROW_BTH)
                             : tile_grid(w, h, BDPT_AOV_BVH_BTW, BDPT_AOV_BVH_BTH);
    if (timed)
        if (int rc = svc_begin(c, kSvcChain)) return rc;
    hipLaunchKernelGGL(bdpt_chain_kernel, grid, dim3(256), 0, c->stream, a, v);
    HIPCHK(c, hipGetLastError());
    if (timed)
        if (int rc = svc_end(c, kSvcChain)) return rc;
    *vout = v;
    return BDPT_OK;
}
// The denoisers' guide planes of the whole frame, by `materials`: the unjittered first hit, or
// (BDPT_DENOISE_THROUGH) the key and end normal of the unjittered TRANSMIT chain.  *all: what the
// pack kernels' all_materials is -- a key is an eligible guide as it stands.
static int guide_frame(bdpt_ctx* c, int materials, const int** id, const bdpt_dev_vec** normal, int* all) {
    if (materials == BDPT_DENOISE_THROUGH) {
        bdpt_chain_args cv;
        if (int rc = chain_launch(c, 0, 0, c->W, c->H, 0, 0u, BDPT_CHAIN_TRANSMIT, true, false, &cv)) return rc;
        *id = cv.id; *normal = cv.normal; *all = 1;
        return BDPT_OK;
    }
    bdpt_aov_args av;
    if (int rc = aov_frame(c, c->cam, &av)) return rc;
    *id = av.id; *normal = av.normal; *all = materials == BDPT_DENOISE_ALL;
    return BDPT_OK;
}
// bdpt_denoise / bdpt_denoise_noise: the `materials` values they take; "through" keys must fit an int
static int materials_check(bdpt_ctx* c, const char* who, int materials) {
    if (materials != BDPT_DENOISE_DIFFUSE && materials != BDPT_DENOISE_ALL && materials != BDPT_DENOISE_THROUGH)
        return fail(c, BDPT_EINVAL, "%s: materials %d", who, materials);
    if (materials == BDPT_DENOISE_THROUGH && !bdpt_chain_keys_fit((unsigned)c->spheres.size()))
        return fail(c, BDPT_EINVAL, "%s: %zu spheres are too many for the guide keys of materials = through", who,
                    c->spheres.size());
    return BDPT_OK;
}

// The packed results of a call, on the device: what the last kernel writes and the read-back
// copies.  wanted(): those of `have` the caller gave a host buffer for, nullptr for the others.
struct frame_outs {
    bdpt_dev_vec* out3;
    float* weight;
    uchar4* rgba;
};
static frame_outs wanted(const frame_outs& have, const void* colors_out, const void* weight_out, const void* rgba_out) {
    return {colors_out ? have.out3 : nullptr, weight_out ? have.weight : nullptr, rgba_out ? have.rgba : nullptr};
}
static void set_outs(bdpt_denoise_args& v, const frame_outs& o) { v.out3 = o.out3; v.rgba = o.rgba; }
// (the noise-guided denoiser's variance plane travels in the `weight` slot)
static void set_outs(bdpt_dnoise_args& v, const frame_outs& o) { v.out3 = o.out3; v.variance = o.weight; v.rgba = o.rgba; }
template <class Args>
static void set_outs(Args& v, const frame_outs& o) { v.out3 = o.out3; v.weight = o.weight; v.rgba = o.rgba; }

// The end of a call that wrote `want`: the read-back through the stream, then the frame's verdict.
static int read_outs(bdpt_ctx* c, const frame_outs& want, bdpt_vec* colors_out, float* weight_out,
                     unsigned char* rgba_out) {
    const size_t np = (size_t)c->W * c->H;
    if (want.out3) HIPCHK(c, hipMemcpyAsync(colors_out, want.out3, sizeof(bdpt_vec) * np, hipMemcpyDeviceToHost, c->stream));
    if (want.weight) HIPCHK(c, hipMemcpyAsync(weight_out, want.weight, sizeof(float) * np, hipMemcpyDeviceToHost, c->stream));
    if (want.rgba) HIPCHK(c, hipMemcpyAsync(rgba_out, want.rgba, 4 * np, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return units_verdict(c);                                 // a frame known to be invalid is an error
}

// d_dn: the denoiser's guide, ping and pong records (bdpt_denoise and bdpt_preview_denoise)
struct dn_bufs {
    float4 *guide, *ping, *pong;
};
static int dn_alloc(bdpt_ctx* c, const char* who, dn_bufs* d) {
    const size_t np = (size_t)c->W * c->H;
    if (!c->d_dn && hipMalloc(&c->d_dn, 3 * sizeof(float4) * np) != hipSuccess) {
        c->d_dn = nullptr;
        return fail(c, BDPT_ENOMEM, "%s: guide, ping and pong buffers (%zu B)", who, 3 * sizeof(float4) * np);
    }
    *d = {c->d_dn, c->d_dn + np, c->d_dn + 2 * np};
    return BDPT_OK;
}

// The filter parameters bdpt_denoise (1..8 levels) and bdpt_preview_denoise (0..8) share.
static int filter_check(bdpt_ctx* c, const char* who, int levels, int min_levels, int normal_power, float sigma_color) {
    if (levels < min_levels || levels > 8)
        return fail(c, BDPT_EINVAL, "%s: levels %d outside %d..8", who, levels, min_levels);
    if (normal_power < 0 || normal_power > 6)
        return fail(c, BDPT_EINVAL, "%s: normal_power %d outside 0..6", who, normal_power);
    if (!(sigma_color > 0.f)) return fail(c, BDPT_EINVAL, "%s: sigma_color must be > 0", who);
    return BDPT_OK;
}

// The a-trous levels of either filter: one launch of table[LDS staging][normal_power] per level,
// ping-pong from d.ping, the last of which writes `want` instead of the next buffer.  v arrives
// zeroed but for the fields only its own kernels have.  Tile shape and LDS staging are the measured
// choice; the environment overrides it for experiments (BDPT_DENOISE_TILE = 8 / 64,
// BDPT_DENOISE_LDS = 0 / 1).
template <class Args>
static int run_levels(bdpt_ctx* c, Args& v, const void* (&table)[2][7], int levels, int normal_power,
                      float sigma_color, const dn_bufs& d, const frame_outs& want) {
    v.W = c->W; v.H = c->H;
    v.guide = d.guide;
    v.gamma_thr = c->d_thr;
    v.rows = 1;
    bool lds = true;
    if (const char* e = getenv("BDPT_DENOISE_TILE")) v.rows = atoi(e) == 64;
    if (const char* e = getenv("BDPT_DENOISE_LDS")) lds = atoi(e) == 1;
    const float isc0 = 1.0f / (sigma_color * sigma_color);
    for (int k = 0; k < levels; k++) {
        const bool last = k == levels - 1;
        v.step = 1 << k;
        v.isc = isc0 * (float)(1 << (2 * k));
        v.cur = k % 2 ? d.pong : d.ping;
        v.nxt = last ? nullptr : (k % 2 ? d.ping : d.pong);
        if (last) set_outs(v, want);
        const bool staged = lds && v.step <= BDPT_DN_LDS_MAX_STEP;
        const dim3 grid = staged || !v.rows ? tile_grid(c->W, c->H, BDPT_DN_BTW, BDPT_DN_BTH)
                                            : tile_grid(c->W, c->H, BDPT_DN_ROW_BTW, BDPT_DN_ROW_BTH);
        void* kargs[] = {&v};
        HIPCHK(c, hipLaunchKernel(table[staged][normal_power], grid, dim3(256), kargs, 0, c->stream));
    }
    return BDPT_OK;
}

// ---- first-hit feature buffers (include/bdpt.h bdpt_render_aov) -----------------------------
// One launch of bdpt_aov_kernel over the window on the context's stream (so it runs after the
// table generation, light pass and scene upload queued there; it reads nothing the path passes
// write), then the wanted planes are read back through the same stream.
int bdpt_render_aov(bdpt_ctx* c, int x0, int y0, int w, int h, int jitter, unsigned sid,
                    const bdpt_aov_buffers* out) {
    if (!c) return BDPT_EINVAL;
    if (c->multi) return fail(c, BDPT_EINVAL, "bdpt_render_aov: multi-device contexts render no feature buffers");
    if (!out) return fail(c, BDPT_EINVAL, "bdpt_render_aov: no output buffers");
    if (w <= 0 || h <= 0 || x0 < 0 || y0 < 0 || x0 > c->W - w || y0 > c->H - h)
        return fail(c, BDPT_EINVAL, "bdpt_render_aov: window %d,%d %dx%d is empty or outside the %dx%d frame", x0, y0,
                    w, h, c->W, c->H);
    if (sid >= (unsigned)BDPT_RAND_N) return fail(c, BDPT_EINVAL, "bdpt_render_aov: sid %u >= RAND_N", sid);
    if (!c->cam_set) return fail(c, BDPT_ESTATE, "bdpt_render_aov: camera not set");
    if (jitter && !c->rand_ready)
        return fail(c, BDPT_ESTATE, "bdpt_render_aov: jitter needs a random table (run the light pass first)");
    if (c->cpu) {
        svc_cpu(c, kSvcAov, [&] { bdpt_cpu_render_aov(c->cpu, x0, y0, w, h, jitter, sid, out); });
        c->aov_traversal = BDPT_TRAVERSE_BRUTE;
        return BDPT_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    const size_t np = (size_t)w * (size_t)h;
    bdpt_aov_args v;
    if (int rc = aov_launch(c, c->cam, x0, y0, w, h, jitter, sid, true, &v)) return rc;
    c->aov_traversal = v.bvh ? BDPT_TRAVERSE_BVH : BDPT_TRAVERSE_BRUTE;
    auto back = [&](void* dst, const void* src, size_t bytes) -> hipError_t {
        return dst ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream) : hipSuccess;
    };
    HIPCHK(c, back(out->id, v.id, sizeof(int) * np));
    HIPCHK(c, back(out->t, v.t, sizeof(float) * np));
    HIPCHK(c, back(out->dp, v.dp, sizeof(float) * np));
    HIPCHK(c, back(out->position, v.position, sizeof(bdpt_vec) * np));
    HIPCHK(c, back(out->normal, v.normal, sizeof(bdpt_vec) * np));
    HIPCHK(c, back(out->dir, v.dir, sizeof(bdpt_vec) * np));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BDPT_OK;
}

int bdpt_pick(bdpt_ctx* c, int x, int y, int jitter, unsigned sid, int* id, float* t) {
    bdpt_aov_buffers out;
    memset(&out, 0, sizeof(out));
    out.id = id;
    out.t = t;
    return bdpt_render_aov(c, x, y, 1, 1, jitter, sid, &out);
}

int bdpt_last_aov_traversal(const bdpt_ctx* c) {
    if (!c) return BDPT_EINVAL;
    return c->aov_traversal ? c->aov_traversal : BDPT_ESTATE;
}

int bdpt_last_aov_ms(bdpt_ctx* c, float* ms) {
    return svc_last_ms(c, kSvcAov, ms, "bdpt_last_aov_ms: no feature buffers rendered");
}

// ---- the eye path up to its first non-specular vertex (include/bdpt.h bdpt_render_chain;
// DESIGN.md 4j) -----------------------------------------------------------------------------
// bdpt_render_aov's sequence with bdpt_chain_kernel and its ten planes in d_chain.
int bdpt_render_chain(bdpt_ctx* c, int x0, int y0, int w, int h, int jitter, unsigned sid, int branch,
                      const bdpt_chain_buffers* out) {
    if (!c) return BDPT_EINVAL;
    if (c->multi) return fail(c, BDPT_EINVAL, "bdpt_render_chain: multi-device contexts render no feature buffers");
    if (!out) return fail(c, BDPT_EINVAL, "bdpt_render_chain: no output buffers");
    if (w <= 0 || h <= 0 || x0 < 0 || y0 < 0 || x0 > c->W - w || y0 > c->H - h)
        return fail(c, BDPT_EINVAL, "bdpt_render_chain: window %d,%d %dx%d is empty or outside the %dx%d frame", x0,
                    y0, w, h, c->W, c->H);
    if (sid >= (unsigned)BDPT_RAND_N) return fail(c, BDPT_EINVAL, "bdpt_render_chain: sid %u >= RAND_N", sid);
    if (branch != BDPT_CHAIN_TRANSMIT && branch != BDPT_CHAIN_PASS)
        return fail(c, BDPT_EINVAL, "bdpt_render_chain: branch %d", branch);
    if (branch == BDPT_CHAIN_PASS && !jitter)
        return fail(c, BDPT_EINVAL, "bdpt_render_chain: BDPT_CHAIN_PASS is the choice of a pass: it needs jitter");
    if (!c->cam_set) return fail(c, BDPT_ESTATE, "bdpt_render_chain: camera not set");
    if (jitter && !c->rand_ready)
        return fail(c, BDPT_ESTATE, "bdpt_render_chain: jitter needs a random table (run the light pass first)");
    if (c->cpu) {
        svc_cpu(c, kSvcChain, [&] { bdpt_cpu_render_chain(c->cpu, x0, y0, w, h, jitter, sid, branch, out); });
        return BDPT_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    const size_t np = (size_t)w * (size_t)h;
    bdpt_chain_args v;
    if (int rc = chain_launch(c, x0, y0, w, h, jitter, sid, branch, false, true, &v)) return rc;
    auto back = [&](void* dst, const void* src, size_t bytes) -> hipError_t {
        return dst ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream) : hipSuccess;
    };
    HIPCHK(c, back(out->id, v.id, sizeof(int) * np));
    HIPCHK(c, back(out->first_id, v.first_id, sizeof(int) * np));
    HIPCHK(c, back(out->kind, v.kind, sizeof(int) * np));
    HIPCHK(c, back(out->bounces, v.bounces, sizeof(int) * np));
    HIPCHK(c, back(out->t, v.t, sizeof(float) * np));
    HIPCHK(c, back(out->dp, v.dp, sizeof(float) * np));
    HIPCHK(c, back(out->position, v.position, sizeof(bdpt_vec) * np));
    HIPCHK(c, back(out->normal, v.normal, sizeof(bdpt_vec) * np));
    HIPCHK(c, back(out->dir, v.dir, sizeof(bdpt_vec) * np));
    HIPCHK(c, back(out->throughput, v.throughput, sizeof(bdpt_vec) * np));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BDPT_OK;
}

int bdpt_last_chain_ms(bdpt_ctx* c, float* ms) {
    return svc_last_ms(c, kSvcChain, ms, "bdpt_last_chain_ms: no chain rendered");
}

// ---- edge-avoiding wavelet denoiser (include/bdpt.h bdpt_denoise) --------------
// The guides (the unjittered whole-frame bdpt_aov_kernel, or bdpt_chain_kernel's keys for
// materials = through), bdpt_denoise_pack_kernel (guide records + the first ping buffer), the levels, then the read-back.  The packed results go where the feature planes
// were: the pack kernel has consumed them, and 16 B of a pixel's 48 B there hold its float3 and
// its RGBA.  Only d_aov and d_dn are written.
int bdpt_denoise(bdpt_ctx* c, const bdpt_denoise_params* p, bdpt_vec* colors_out, unsigned char* rgba_out) {
    if (!c) return BDPT_EINVAL;
    if (c->multi) return fail(c, BDPT_EINVAL, "bdpt_denoise: multi-device contexts are not denoised (upload the assembled frame to a one-device context)");
    if (!p) return fail(c, BDPT_EINVAL, "bdpt_denoise: no parameters");
    if (!colors_out && !rgba_out) return fail(c, BDPT_EINVAL, "bdpt_denoise: no output buffer");
    if (int rc = filter_check(c, "bdpt_denoise", p->levels, 1, p->normal_power, p->sigma_color)) return rc;
    if (int rc = materials_check(c, "bdpt_denoise", p->materials)) return rc;
    if (!c->cam_set) return fail(c, BDPT_ESTATE, "bdpt_denoise: camera not set");
    if (c->cpu) {
        svc_cpu(c, kSvcDenoise, [&] { bdpt_cpu_denoise(c->cpu, p, colors_out, rgba_out); });
        return BDPT_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    const size_t np = (size_t)c->W * c->H;
    dn_bufs d;
    if (int rc = dn_alloc(c, "bdpt_denoise", &d)) return rc;
    if (int rc = join_fold(c)) return rc;
    if (int rc = svc_begin(c, kSvcDenoise)) return rc;
    const int* gid;
    const bdpt_dev_vec* gnormal;
    int all;
    if (int rc = guide_frame(c, p->materials, &gid, &gnormal, &all)) return rc;
    hipLaunchKernelGGL(bdpt_denoise_pack_kernel, lane_grid(np), dim3(256), 0, c->stream, gid, gnormal,
                       (const bdpt_dev_vec*)c->d_colors, (const bdpt_dev_sphere*)c->d_sph, all, d.guide, d.ping, (int)np);
    HIPCHK(c, hipGetLastError());
    // 3 of a pixel's 12 words in d_aov, and the 4th
    const frame_outs want = wanted({(bdpt_dev_vec*)c->d_aov, nullptr, (uchar4*)(c->d_aov + 3 * c->aov_cap)}, colors_out,
                                   nullptr, rgba_out);
    bdpt_denoise_args v;
    memset(&v, 0, sizeof(v));
    v.normal_power = p->normal_power;
    if (int rc = run_levels(c, v, bdpt_denoise_level_table, p->levels, p->normal_power, p->sigma_color, d, want)) return rc;
    if (int rc = svc_end(c, kSvcDenoise)) return rc;
    return read_outs(c, want, colors_out, nullptr, rgba_out);
}

int bdpt_last_denoise_ms(bdpt_ctx* c, float* ms) {
    return svc_last_ms(c, kSvcDenoise, ms, "bdpt_last_denoise_ms: no frame denoised");
}

// ---- noise-guided denoiser (include/bdpt.h bdpt_denoise_noise) ------------------
// bdpt_denoise's sequence with the variance in the colour records' .w: the unjittered whole-frame
// bdpt_aov_kernel, bdpt_dnoise_pack_kernel (guide records + {B, raw variance} into ping),
// bdpt_dnoise_prefilter_kernel (ping -> pong), the levels from pong, then the read-back.  The packed
// results go where the feature planes were, the variance plane into the 5th word of a pixel's 12
// there.  The mark is only read (a context without one: every pixel without an estimate).  Only
// d_aov and d_dn are written.
int bdpt_denoise_noise(bdpt_ctx* c, const bdpt_denoise_noise_params* p, bdpt_vec* colors_out, unsigned char* rgba_out,
                       float* variance_out) {
    if (!c) return BDPT_EINVAL;
    if (c->multi) return fail(c, BDPT_EINVAL, "bdpt_denoise_noise: multi-device contexts are not denoised (upload the assembled frame to a one-device context)");
    if (!p) return fail(c, BDPT_EINVAL, "bdpt_denoise_noise: no parameters");
    if (!colors_out && !rgba_out) return fail(c, BDPT_EINVAL, "bdpt_denoise_noise: no output buffer");
    if (int rc = filter_check(c, "bdpt_denoise_noise", p->levels, 1, p->normal_power, p->sigma_color)) return rc;
    if (int rc = materials_check(c, "bdpt_denoise_noise", p->materials)) return rc;
    if (!(p->noise_sigma > 0.f && p->noise_sigma < INFINITY))
        return fail(c, BDPT_EINVAL, "bdpt_denoise_noise: noise_sigma must be > 0 and finite");
    if (!c->cam_set) return fail(c, BDPT_ESTATE, "bdpt_denoise_noise: camera not set");
    if (c->cpu) {
        svc_cpu(c, kSvcDenoiseNoise, [&] { bdpt_cpu_denoise_noise(c->cpu, p, colors_out, rgba_out, variance_out); });
        return BDPT_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    const size_t np = (size_t)c->W * c->H;
    dn_bufs d;
    if (int rc = dn_alloc(c, "bdpt_denoise_noise", &d)) return rc;
    if (int rc = join_fold(c)) return rc;
    if (int rc = svc_begin(c, kSvcDenoiseNoise)) return rc;
    const int* gid;
    const bdpt_dev_vec* gnormal;
    int all;
    if (int rc = guide_frame(c, p->materials, &gid, &gnormal, &all)) return rc;
    hipLaunchKernelGGL(bdpt_dnoise_pack_kernel, lane_grid(np), dim3(256), 0, c->stream, gid, gnormal,
                       (const bdpt_dev_vec*)c->d_colors, (const unsigned*)c->d_counter,
                       (const uint4*)c->d_mark, (int)c->mark_live, (const bdpt_dev_sphere*)c->d_sph, all, d.guide,
                       d.ping, (int)np);
    HIPCHK(c, hipGetLastError());
    // (experiments: BDPT_DNOISE_PREFILTER=0 leaves the prefilter out -- the levels then read the raw
    // variances, which is not the definition -- so that scripts/denoise_noise_time.py can time its share)
    bool prefilter = true;
    if (const char* e = getenv("BDPT_DNOISE_PREFILTER")) prefilter = atoi(e) != 0;
    if (prefilter) {
        hipLaunchKernelGGL(bdpt_dnoise_prefilter_kernel, tile_grid(c->W, c->H, BDPT_DN_BTW, BDPT_DN_BTH), dim3(256), 0,
                           c->stream, (const float4*)d.guide, (const float4*)d.ping, d.pong, c->W, c->H);
        HIPCHK(c, hipGetLastError());
    }
    // words 0..2 of a pixel's 12 in d_aov, the 4th and the 5th
    const frame_outs want = wanted({(bdpt_dev_vec*)c->d_aov, c->d_aov + 4 * c->aov_cap, (uchar4*)(c->d_aov + 3 * c->aov_cap)},
                                   colors_out, variance_out, rgba_out);
    bdpt_dnoise_args v;
    memset(&v, 0, sizeof(v));
    v.s2 = p->noise_sigma * p->noise_sigma;
    const dn_bufs from_pong = {d.guide, d.pong, d.ping};     // the levels start at the prefilter's output
    if (int rc = run_levels(c, v, bdpt_dnoise_level_table, p->levels, p->normal_power, p->sigma_color,
                            prefilter ? from_pong : d, want))
        return rc;
    if (int rc = svc_end(c, kSvcDenoiseNoise)) return rc;
    return read_outs(c, want, colors_out, variance_out, rgba_out);
}

int bdpt_last_denoise_noise_ms(bdpt_ctx* c, float* ms) {
    return svc_last_ms(c, kSvcDenoiseNoise, ms, "bdpt_last_denoise_noise_ms: no frame denoised");
}

// ---- temporal reprojection (include/bdpt.h bdpt_reproject) ---------------------
// The unjittered whole-frame bdpt_aov_kernel under the current camera, (capture)
// bdpt_history_pack_kernel writing the next history's guide records from its planes, then
// bdpt_reproject_kernel, which reads the history's records and writes the packed results or the
// next history's colour records; then the read-back.  Only d_aov and d_hist are written.
// The state of the stored history against the context's spheres (BDPT_HISTORY_*; delta: one offset
// per sphere in the states SAME and MOVED, or nullptr), and whether a history in that state is present.
static int hist_state(const bdpt_ctx* c, bdpt_vec* delta) {
    if (c->cpu) return bdpt_cpu_history_motion(c->cpu, delta);
    return bdpt_history_state(c->has_hist, c->hist_spheres.data(), c->hist_spheres.size(), c->spheres.data(),
                              c->spheres.size(), delta);
}
static bool hist_present(const bdpt_ctx* c, int state) {
    return state == BDPT_HISTORY_SAME || (c->hist_follow && state == BDPT_HISTORY_MOVED);
}
static bool hist_present(const bdpt_ctx* c) { return hist_present(c, hist_state(c, nullptr)); }

// What a call finds of the history: whether one is present, and ("follow", some sphere moved) the
// table of offsets in d_hdelta, one float4 per sphere.  The table is written here, with the state,
// when the offsets are not the ones it holds -- once per sphere move, before the service's clock
// starts.  The copy's source is hdelta_up, which stands until the next move.
struct hist_use {
    bool present;
    const float4* hdelta;
};
static int hist_eval(bdpt_ctx* c, hist_use* u) {
    const size_t n = c->spheres.size();
    std::vector<bdpt_vec> delta(c->hist_follow ? n : 0);
    const int state = hist_state(c, delta.empty() ? nullptr : delta.data());
    u->present = hist_present(c, state);
    u->hdelta = nullptr;
    if (!c->hist_follow || state != BDPT_HISTORY_MOVED) return BDPT_OK;
    std::vector<float4> table(n);
    for (size_t k = 0; k < n; k++) table[k] = make_float4(delta[k].x, delta[k].y, delta[k].z, 0.f);
    const bool held = c->d_hdelta && c->hdelta_up.size() == n &&
                      memcmp(c->hdelta_up.data(), table.data(), sizeof(float4) * n) == 0;
    if (!held) {
        if (c->hdelta_up.size() != n || !c->d_hdelta) {
            HIPCHK(c, hipStreamSynchronize(c->stream));           // an earlier call's kernels are done anyway
            if (c->d_hdelta) HIPCHK(c, hipFree(c->d_hdelta));
            c->d_hdelta = nullptr;
            c->hdelta_up.clear();
            if (hipMalloc(&c->d_hdelta, sizeof(float4) * n) != hipSuccess) {
                c->d_hdelta = nullptr;
                return fail(c, BDPT_ENOMEM, "bdpt_reproject: the followed spheres' offsets (%zu B)", sizeof(float4) * n);
            }
        }
        c->hdelta_up.swap(table);
        HIPCHK(c, hipMemcpyAsync(c->d_hdelta, c->hdelta_up.data(), sizeof(float4) * n, hipMemcpyHostToDevice, c->stream));
    }
    u->hdelta = c->d_hdelta;
    return BDPT_OK;
}

static int rp_check(bdpt_ctx* c, const bdpt_reproject_params* p, const char* who) {
    if (c->multi) return fail(c, BDPT_EINVAL, "%s: multi-device contexts keep no history", who);
    if (!p) return fail(c, BDPT_EINVAL, "%s: no parameters", who);
    if (p->materials != BDPT_DENOISE_DIFFUSE && p->materials != BDPT_DENOISE_ALL)
        return fail(c, BDPT_EINVAL, "%s: materials %d", who, p->materials);
    if (!(p->max_history > 0.f)) return fail(c, BDPT_EINVAL, "%s: max_history must be > 0", who);
    if (!(p->plane_tol >= 0.f)) return fail(c, BDPT_EINVAL, "%s: plane_tol must be >= 0", who);
    return BDPT_OK;
}

// d_hist: float4[4][np] (set s: guide at 2 s, colour + weight at 2 s + 1), then out3, weight, rgba
struct hist_bufs {
    float4 *guide[2], *col[2];
    frame_outs res;
};
static int hist_alloc(bdpt_ctx* c, hist_bufs* b) {
    const size_t np = (size_t)c->W * c->H, bytes = (4 * sizeof(float4) + sizeof(bdpt_dev_vec) + sizeof(float) + 4) * np;
    if (!c->d_hist && hipMalloc(&c->d_hist, bytes) != hipSuccess) {
        c->d_hist = nullptr;
        return fail(c, BDPT_ENOMEM, "bdpt_reproject: history and result buffers (%zu B)", bytes);
    }
    for (int s = 0; s < 2; s++) {
        b->guide[s] = c->d_hist + 2 * s * np;
        b->col[s] = c->d_hist + (2 * s + 1) * np;
    }
    b->res.out3 = (bdpt_dev_vec*)(c->d_hist + 4 * np);
    b->res.weight = (float*)(b->res.out3 + np);
    b->res.rgba = (uchar4*)(b->res.weight + np);
    return BDPT_OK;
}

// bdpt_reproject_kernel's arguments but for its outputs: the current view's first hit (av), the
// frame, and the history present, if any (hist_eval's answer)
static bdpt_reproject_args rp_args(bdpt_ctx* c, const bdpt_reproject_params* p, const bdpt_aov_args& av,
                                   const hist_bufs& b, const hist_use& u) {
    bdpt_reproject_args v;
    memset(&v, 0, sizeof(v));
    v.W = c->W; v.H = c->H;
    v.all_materials = p->materials == BDPT_DENOISE_ALL;
    v.max_history = p->max_history;
    v.plane_tol = p->plane_tol;
    v.id = av.id; v.t = av.t; v.position = av.position; v.normal = av.normal;
    v.sph = c->d_sph;
    v.colors = c->d_colors;
    v.counter = c->d_counter;
    v.gamma_thr = c->d_thr;
    if (u.present) {
        bdpt_path_args ha;                                    // C0 as the kernels' camera constants
        memset(&ha, 0, sizeof(ha));
        camera_args(c, c->hist_cam, ha);
        memcpy(v.ux, ha.ux, sizeof(v.ux)); memcpy(v.uy, ha.uy, sizeof(v.uy)); memcpy(v.ud, ha.ud, sizeof(v.ud));
        memcpy(v.o, ha.orig, sizeof(v.o));
        v.hw = (float)ha.half_w; v.hh = (float)ha.half_h;
        v.sx = 1.f / ha.inv_w; v.sy = 1.f / ha.inv_h;
        v.hguide = b.guide[c->hist_cur];
        v.hcol = b.col[c->hist_cur];
        v.hdelta = u.hdelta;
    }
    // wave tile: the measured choice; BDPT_REPROJECT_TILE = 8 / 64 overrides it
    v.rows = 1;
    if (const char* e = getenv("BDPT_REPROJECT_TILE")) v.rows = atoi(e) != 8;
    return v;
}

// the history under `cam` is the set hist_cur
static void hist_stored(bdpt_ctx* c, const bdpt_camera& cam) {
    c->has_hist = true;
    c->hist_cam = cam;
    c->hist_spheres = c->spheres;
}

// bdpt_reproject, bdpt_history_capture (`capture`) and bdpt_preview_denoise (`pv`), which differ in
// where bdpt_reproject_kernel's result goes: the packed results, the next history's records, or
// (pv->levels > 0) the denoiser's ping buffer for the count-aware levels that follow.
static int rp_run(bdpt_ctx* c, const bdpt_reproject_params* p, bool capture, const bdpt_preview_params* pv,
                  bdpt_vec* colors_out, float* weight_out, unsigned char* rgba_out) {
    const int svc = pv ? kSvcPreview : kSvcReproject;
    if (c->cpu) {
        svc_cpu(c, svc, [&] {
            if (capture) bdpt_cpu_history_capture(c->cpu, p);
            else if (pv) bdpt_cpu_preview_denoise(c->cpu, pv, colors_out, weight_out, rgba_out);
            else bdpt_cpu_reproject(c->cpu, p, colors_out, weight_out, rgba_out);
        });
        return BDPT_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    const size_t np = (size_t)c->W * c->H;
    hist_bufs b;
    if (int rc = hist_alloc(c, &b)) return rc;
    dn_bufs d{};
    if (pv)
        if (int rc = dn_alloc(c, "bdpt_preview_denoise", &d)) return rc;
    hist_use use;
    if (int rc = hist_eval(c, &use)) return rc;
    if (int rc = join_fold(c)) return rc;
    if (int rc = svc_begin(c, svc)) return rc;
    bdpt_aov_args av;
    if (int rc = aov_frame(c, c->cam, &av)) return rc;
    const int nxt = c->hist_cur ^ 1;
    bdpt_reproject_args v = rp_args(c, p, av, b, use);
    const frame_outs want = wanted(b.res, colors_out, weight_out, rgba_out);   // a capture wants none
    if (capture) {
        hipLaunchKernelGGL(bdpt_history_pack_kernel, lane_grid(np), dim3(256), 0, c->stream, (const int*)av.id,
                           (const bdpt_dev_vec*)av.position, (const bdpt_dev_vec*)nullptr, (const float*)nullptr,
                           b.guide[nxt], (float4*)nullptr, (int)np);
        HIPCHK(c, hipGetLastError());
        v.next = b.col[nxt];
    } else if (!pv || pv->levels == 0) {
        set_outs(v, want);
    } else {
        // the {o, clampc(tot)} record goes into the ping buffer and the guide record into the guide
        // buffer (BDPT_PREVIEW_GUIDE=pack: bdpt_denoise_pack_kernel writes the guide records instead,
        // the alternative that was measured)
        const char* e = getenv("BDPT_PREVIEW_GUIDE");
        if (e && strcmp(e, "pack") == 0) {
            hipLaunchKernelGGL(bdpt_denoise_pack_kernel, lane_grid(np), dim3(256), 0, c->stream, (const int*)av.id,
                               (const bdpt_dev_vec*)av.normal, (const bdpt_dev_vec*)nullptr,
                               (const bdpt_dev_sphere*)c->d_sph, v.all_materials, d.guide, (float4*)nullptr, (int)np);
            HIPCHK(c, hipGetLastError());
        } else {
            v.dn_guide = d.guide;
        }
        v.next = d.ping;
        v.clamp_next = 1;
    }
    const dim3 grid = v.rows ? tile_grid(c->W, c->H, BDPT_RP_ROW_BTW, BDPT_RP_ROW_BTH)
                             : tile_grid(c->W, c->H, BDPT_RP_BTW, BDPT_RP_BTH);
    hipLaunchKernelGGL(bdpt_reproject_kernel, grid, dim3(256), 0, c->stream, v);
    HIPCHK(c, hipGetLastError());
    if (pv) {
        bdpt_preview_args lv;
        memset(&lv, 0, sizeof(lv));
        lv.c2 = 2.f / pv->count_ref;
        if (int rc = run_levels(c, lv, bdpt_preview_level_table, pv->levels, pv->normal_power, pv->sigma_color, d, want))
            return rc;
    }
    if (int rc = svc_end(c, svc)) return rc;
    if (capture) {
        c->hist_cur = nxt;
        hist_stored(c, c->cam);
    }
    return read_outs(c, want, colors_out, weight_out, rgba_out);
}

int bdpt_reproject(bdpt_ctx* c, const bdpt_reproject_params* p, bdpt_vec* colors_out, float* weight_out,
                   unsigned char* rgba_out) {
    if (!c) return BDPT_EINVAL;
    if (int rc = rp_check(c, p, "bdpt_reproject")) return rc;
    if (!colors_out && !weight_out && !rgba_out) return fail(c, BDPT_EINVAL, "bdpt_reproject: no output buffer");
    if (!c->cam_set) return fail(c, BDPT_ESTATE, "bdpt_reproject: camera not set");
    return rp_run(c, p, false, nullptr, colors_out, weight_out, rgba_out);
}

int bdpt_history_capture(bdpt_ctx* c, const bdpt_reproject_params* p) {
    if (!c) return BDPT_EINVAL;
    if (int rc = rp_check(c, p, "bdpt_history_capture")) return rc;
    if (!c->cam_set) return fail(c, BDPT_ESTATE, "bdpt_history_capture: camera not set");
    return rp_run(c, p, true, nullptr, nullptr, nullptr, nullptr);
}

int bdpt_history_clear(bdpt_ctx* c) {
    if (!c) return BDPT_EINVAL;
    if (c->multi) return fail(c, BDPT_EINVAL, "bdpt_history_clear: multi-device contexts keep no history");
    if (c->cpu) bdpt_cpu_history_clear(c->cpu);
    c->has_hist = false;
    return BDPT_OK;
}

int bdpt_history_follow(bdpt_ctx* c, int on) {
    if (!c) return BDPT_EINVAL;
    if (c->multi) return fail(c, BDPT_EINVAL, "bdpt_history_follow: multi-device contexts keep no history");
    if (c->cpu) bdpt_cpu_history_follow(c->cpu, on);
    c->hist_follow = on != 0;
    return BDPT_OK;
}

int bdpt_history_motion(const bdpt_ctx* c, int* state, bdpt_vec* delta, unsigned n) {
    if (!c || c->multi) return BDPT_EINVAL;
    if (delta && n != c->spheres.size()) return BDPT_EINVAL;
    const int s = hist_state(c, delta);
    if (state) *state = s;
    return BDPT_OK;
}

int bdpt_history_info(const bdpt_ctx* c, int* present, bdpt_camera* camera) {
    if (!c || c->multi) return BDPT_EINVAL;
    if (present) *present = hist_present(c);
    if (c->cpu) (void)bdpt_cpu_history_stored(c->cpu, camera);
    else if (c->has_hist && camera) *camera = c->hist_cam;
    return BDPT_OK;
}

int bdpt_history_read(bdpt_ctx* c, bdpt_vec* colors, float* weight) {
    if (!c) return BDPT_EINVAL;
    if (c->multi) return fail(c, BDPT_EINVAL, "bdpt_history_read: multi-device contexts keep no history");
    if (!colors && !weight) return fail(c, BDPT_EINVAL, "bdpt_history_read: no output buffer");
    if (!(c->cpu ? bdpt_cpu_history_stored(c->cpu, nullptr) : c->has_hist))
        return fail(c, BDPT_ESTATE, "bdpt_history_read: no history");
    if (c->cpu) {
        bdpt_cpu_history_read(c->cpu, colors, weight);
        return BDPT_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    const size_t np = (size_t)c->W * c->H;
    hist_bufs b;
    if (int rc = hist_alloc(c, &b)) return rc;
    std::vector<float4> rec(np);
    HIPCHK(c, hipMemcpyAsync(rec.data(), b.col[c->hist_cur], sizeof(float4) * np, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < np; i++) {
        if (colors) colors[i] = {rec[i].x, rec[i].y, rec[i].z};
        if (weight) weight[i] = rec[i].w;
    }
    return BDPT_OK;
}

int bdpt_history_write(bdpt_ctx* c, const bdpt_camera* camera, const bdpt_vec* colors, const float* weight) {
    if (!c) return BDPT_EINVAL;
    if (c->multi) return fail(c, BDPT_EINVAL, "bdpt_history_write: multi-device contexts keep no history");
    if (!camera || !colors || !weight) return fail(c, BDPT_EINVAL, "bdpt_history_write: NULL argument");
    if (c->cpu) {
        bdpt_cpu_history_write(c->cpu, camera, colors, weight);
        return BDPT_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    const size_t np = (size_t)c->W * c->H;
    hist_bufs b;
    if (int rc = hist_alloc(c, &b)) return rc;
    if (int rc = join_fold(c)) return rc;
    // staged in the result buffers, then packed with the guides rendered under `camera`
    HIPCHK(c, hipMemcpyAsync(b.res.out3, colors, sizeof(bdpt_vec) * np, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(b.res.weight, weight, sizeof(float) * np, hipMemcpyHostToDevice, c->stream));
    bdpt_aov_args av;
    if (int rc = aov_frame(c, *camera, &av)) return rc;
    hipLaunchKernelGGL(bdpt_history_pack_kernel, lane_grid(np), dim3(256), 0, c->stream, (const int*)av.id,
                       (const bdpt_dev_vec*)av.position, (const bdpt_dev_vec*)b.res.out3, (const float*)b.res.weight,
                       b.guide[c->hist_cur], b.col[c->hist_cur], (int)np);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    hist_stored(c, *camera);
    return BDPT_OK;
}

int bdpt_last_reproject_ms(bdpt_ctx* c, float* ms) {
    return svc_last_ms(c, kSvcReproject, ms, "bdpt_last_reproject_ms: no frame reprojected");
}

// ---- the reprojected preview, denoised with per-pixel counts (include/bdpt.h
// bdpt_preview_denoise) ----------------------------------------------------------
// rp_run with the preview's parameters: bdpt_aov_kernel once, bdpt_reproject_kernel feeding the
// denoiser's buffers, then the count-aware levels, the last of which writes the packed results into
// d_hist's result buffers; then the read-back.  levels == 0 is the reprojection alone.  Only d_aov,
// d_dn and d_hist's result buffers are written.
int bdpt_preview_denoise(bdpt_ctx* c, const bdpt_preview_params* p, bdpt_vec* colors_out, float* weight_out,
                         unsigned char* rgba_out) {
    if (!c) return BDPT_EINVAL;
    if (c->multi) return fail(c, BDPT_EINVAL, "bdpt_preview_denoise: multi-device contexts keep no history");
    if (!p) return fail(c, BDPT_EINVAL, "bdpt_preview_denoise: no parameters");
    if (int rc = rp_check(c, &p->rp, "bdpt_preview_denoise")) return rc;
    if (!colors_out && !weight_out && !rgba_out) return fail(c, BDPT_EINVAL, "bdpt_preview_denoise: no output buffer");
    if (int rc = filter_check(c, "bdpt_preview_denoise", p->levels, 0, p->normal_power, p->sigma_color)) return rc;
    if (!(p->count_ref > 0.f && p->count_ref < INFINITY))
        return fail(c, BDPT_EINVAL, "bdpt_preview_denoise: count_ref must be > 0 and finite");
    if (!c->cam_set) return fail(c, BDPT_ESTATE, "bdpt_preview_denoise: camera not set");
    return rp_run(c, &p->rp, false, p, colors_out, weight_out, rgba_out);
}

int bdpt_last_preview_ms(bdpt_ctx* c, float* ms) {
    return svc_last_ms(c, kSvcPreview, ms, "bdpt_last_preview_ms: no preview denoised");
}

// ---- per-tile noise estimate (include/bdpt.h bdpt_noise_estimate) ---------------
// bdpt_noise_kernel reads colours, counters and the mark's records, writes the tile arrays (and the
// per-pixel plane, and with remark the records of the pixels that take the mark); then the
// read-back, and the summary on the host.  Only d_mark and d_noise are written.
static int nz_check(bdpt_ctx* c, const char* who) {
    if (!c) return BDPT_EINVAL;
    if (c->multi) return fail(c, BDPT_EINVAL, "%s: multi-device contexts keep no mark", who);
    return BDPT_OK;
}

static int mark_alloc(bdpt_ctx* c) {
    if (c->d_mark) return BDPT_OK;
    const size_t bytes = sizeof(uint4) * (size_t)c->W * c->H;
    if (hipMalloc(&c->d_mark, bytes) != hipSuccess) {
        c->d_mark = nullptr;
        return fail(c, BDPT_ENOMEM, "bdpt_noise: mark records (%zu B)", bytes);
    }
    HIPCHK(c, hipMemsetAsync(c->d_mark, 0, bytes, c->stream));
    c->mark_live = false;
    return BDPT_OK;
}

int bdpt_noise_tiles(const bdpt_ctx* c, int* tiles_x, int* tiles_y) {
    if (!c || c->multi) return BDPT_EINVAL;
    if (tiles_x) *tiles_x = (int)cdiv((size_t)c->W, BDPT_NOISE_TW);
    if (tiles_y) *tiles_y = (int)cdiv((size_t)c->H, BDPT_NOISE_TH);
    return BDPT_OK;
}

int bdpt_noise_mark(bdpt_ctx* c) {
    if (int rc = nz_check(c, "bdpt_noise_mark")) return rc;
    if (c->cpu) {
        bdpt_cpu_noise_mark(c->cpu);
        return BDPT_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = mark_alloc(c)) return rc;
    if (int rc = join_fold(c)) return rc;
    const size_t np = (size_t)c->W * c->H;
    hipLaunchKernelGGL(bdpt_noise_mark_kernel, lane_grid(np), dim3(256), 0, c->stream,
                       (const bdpt_dev_vec*)c->d_colors, (const unsigned*)c->d_counter, c->d_mark, (int)np);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->mark_live = true;
    return units_verdict(c);                                 // a frame known to be invalid is an error
}

int bdpt_noise_clear(bdpt_ctx* c) {
    if (int rc = nz_check(c, "bdpt_noise_clear")) return rc;
    if (c->cpu) bdpt_cpu_noise_clear(c->cpu);
    c->mark_live = false;
    return BDPT_OK;
}

int bdpt_noise_read_mark(bdpt_ctx* c, bdpt_vec* colors, unsigned* counter) {
    if (int rc = nz_check(c, "bdpt_noise_read_mark")) return rc;
    if (!colors && !counter) return fail(c, BDPT_EINVAL, "bdpt_noise_read_mark: no output buffer");
    if (!(c->cpu ? bdpt_cpu_noise_stored(c->cpu) : c->d_mark != nullptr))
        return fail(c, BDPT_ESTATE, "bdpt_noise_read_mark: no mark was ever stored");
    if (c->cpu) {
        bdpt_cpu_noise_read_mark(c->cpu, colors, counter);
        return BDPT_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    const size_t np = (size_t)c->W * c->H;
    std::vector<uint4> rec(np);
    HIPCHK(c, hipMemcpyAsync(rec.data(), c->d_mark, sizeof(uint4) * np, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < np; i++) {
        if (colors) memcpy(&colors[i], &rec[i], sizeof(bdpt_vec));
        if (counter) counter[i] = c->mark_live ? rec[i].w : 0u;
    }
    return BDPT_OK;
}

int bdpt_noise_write_mark(bdpt_ctx* c, const bdpt_vec* colors, const unsigned* counter) {
    if (int rc = nz_check(c, "bdpt_noise_write_mark")) return rc;
    if (!colors || !counter) return fail(c, BDPT_EINVAL, "bdpt_noise_write_mark: NULL argument");
    if (c->cpu) {
        bdpt_cpu_noise_write_mark(c->cpu, colors, counter);
        return BDPT_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = mark_alloc(c)) return rc;
    const size_t np = (size_t)c->W * c->H;
    std::vector<uint4> rec(np);
    for (size_t i = 0; i < np; i++) {
        memcpy(&rec[i], &colors[i], sizeof(bdpt_vec));
        rec[i].w = counter[i];
    }
    HIPCHK(c, hipMemcpyAsync(c->d_mark, rec.data(), sizeof(uint4) * np, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->mark_live = true;
    return BDPT_OK;
}

int bdpt_noise_estimate(bdpt_ctx* c, const bdpt_noise_params* p, float* error_out, float* tile_error,
                        unsigned* tile_valid, bdpt_noise_summary* summary) {
    if (int rc = nz_check(c, "bdpt_noise_estimate")) return rc;
    if (!p) return fail(c, BDPT_EINVAL, "bdpt_noise_estimate: no parameters");
    if (!(p->dark > 0.f)) return fail(c, BDPT_EINVAL, "bdpt_noise_estimate: dark must be > 0");
    if (!(p->threshold >= 0.f)) return fail(c, BDPT_EINVAL, "bdpt_noise_estimate: threshold must be >= 0");
    if (!error_out && !tile_error && !tile_valid && !summary)
        return fail(c, BDPT_EINVAL, "bdpt_noise_estimate: no output buffer");
    const size_t np = (size_t)c->W * c->H;
    int tx = 0, ty = 0;
    (void)bdpt_noise_tiles(c, &tx, &ty);
    const size_t nt = (size_t)tx * ty;
    std::vector<unsigned> tiles(4 * nt);                     // S, E (floats), c and the pending count, nt each
    float *S = (float*)tiles.data(), *E = S + nt;
    unsigned *cv = tiles.data() + 2 * nt, *pend = cv + nt;
    if (c->cpu) {
        svc_cpu(c, kSvcNoise, [&] { bdpt_cpu_noise_estimate(c->cpu, p, error_out, S, E, cv, pend); });
    } else {
        HIPCHK(c, hipSetDevice(c->device));
        if (p->remark)
            if (int rc = mark_alloc(c)) return rc;
        const size_t bytes = sizeof(float) * (np + 4 * nt);
        if (!c->d_noise && hipMalloc(&c->d_noise, bytes) != hipSuccess) {
            c->d_noise = nullptr;
            return fail(c, BDPT_ENOMEM, "bdpt_noise_estimate: result buffers (%zu B)", bytes);
        }
        if (int rc = join_fold(c)) return rc;
        bdpt_noise_args v;
        memset(&v, 0, sizeof(v));
        v.W = c->W; v.H = c->H; v.tiles_x = tx;
        v.live = c->mark_live;
        v.remark = p->remark != 0;
        v.dark = p->dark;
        v.colors = c->d_colors;
        v.counter = c->d_counter;
        v.mark = c->d_mark;
        v.error = error_out ? c->d_noise : nullptr;
        v.tile_sum = c->d_noise + np;
        v.tile_error = v.tile_sum + nt;
        v.tile_valid = (unsigned*)(v.tile_error + nt);
        v.tile_pending = v.tile_valid + nt;
        if (int rc = svc_begin(c, kSvcNoise)) return rc;
        hipLaunchKernelGGL(bdpt_noise_kernel, dim3((unsigned)tx, (unsigned)ty, 1), dim3(256), 0, c->stream, v);
        HIPCHK(c, hipGetLastError());
        if (int rc = svc_end(c, kSvcNoise)) return rc;
        if (v.remark) c->mark_live = true;
        if (error_out) HIPCHK(c, hipMemcpyAsync(error_out, v.error, sizeof(float) * np, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(tiles.data(), v.tile_sum, 4 * sizeof(float) * nt, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (int rc = units_verdict(c)) return rc;             // a frame known to be invalid is an error
    }
    if (tile_error) memcpy(tile_error, E, sizeof(float) * nt);
    if (tile_valid) memcpy(tile_valid, cv, sizeof(unsigned) * nt);
    c->noise_pending.assign(pend, pend + nt);
    if (summary) bdpt_noise_summarize(S, E, cv, pend, tx, ty, p->threshold, summary);
    return BDPT_OK;
}

int bdpt_noise_tile_pending(bdpt_ctx* c, unsigned* tile_pending) {
    if (int rc = nz_check(c, "bdpt_noise_tile_pending")) return rc;
    if (!tile_pending) return fail(c, BDPT_EINVAL, "bdpt_noise_tile_pending: no output buffer");
    if (c->noise_pending.empty()) return fail(c, BDPT_ESTATE, "bdpt_noise_tile_pending: no estimate made");
    memcpy(tile_pending, c->noise_pending.data(), sizeof(unsigned) * c->noise_pending.size());
    return BDPT_OK;
}

int bdpt_last_noise_ms(bdpt_ctx* c, float* ms) {
    return svc_last_ms(c, kSvcNoise, ms, "bdpt_last_noise_ms: no estimate made");
}
