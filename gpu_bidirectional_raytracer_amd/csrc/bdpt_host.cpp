// bdpt_host.cpp -- the C-ABI (include/bdpt.h) over the HIP kernels of bdpt_kernels.hip.
//
// Replaces the device-buffer globals and kernel launches of src/smallpt_cpu.c
// (AllocateBuffers :153, FreeBuffers :98, UpdateRendering :265, UpdateRendering2 :300) and
// loadMTGPU/seedMTGPU of src/MersenneTwister_kernel.cu:23-51.  One context = one GPU + one
// HIP stream.  Every HIP call is checked; failures return BDPT_EHIP with the HIP message in
// bdpt_last_error() (the reference prints and continues; the host shell decides).
//
// Here: contexts, scene upload, the path passes, multi-device contexts, checkpoints and the
// display.  The context itself is in bdpt_ctx.h; the run-time compile of the scene-specialised
// path kernels is in bdpt_jit.cpp, and the frame services (feature buffers, denoiser,
// reprojection, preview, noise estimate) are in bdpt_frame.cpp.
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <hip/hip_gl_interop.h>         // hipGraphicsGLRegisterBuffer (the optional display, 8(f)4)
#include <rccl/rccl.h>                 // types and prototypes only: librccl is opened with dlopen
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include <algorithm>
#include <limits>
#include <map>
#include <string>
#include <vector>

#include "bdpt_ctx.h"
#include "bdpt_bvh.h"
#include "bdpt_eye.h"                   // host side: the camera terms
#include <chrono>

using namespace bdpt_host;

static_assert(kBvhEmissive == BDPT_DEV_BVH_EMISSIVE, "BVH id flag");

static_assert(sizeof(bdpt_vec) == 12, "Vec is 12 B (vec.h:4-6)");
static_assert(sizeof(bdpt_ray) == 24, "Ray is 24 B (geom.h:9-11)");
static_assert(sizeof(bdpt_sphere) == 44, "Sphere is 44 B (geom.h:23-27)");
static_assert(sizeof(bdpt_lightpath) == 36, "LightPath is 36 B (geom.h:29-33)");
static_assert(sizeof(bdpt_camera) == 60, "Camera is 60 B (camera.h:7-12)");
static_assert(sizeof(bdpt_dev_lightpath) == sizeof(bdpt_lightpath), "VLP layout");
static_assert(sizeof(bdpt_dev_vec) == sizeof(bdpt_vec), "colour layout");

extern "C" __global__ void bdpt_mt607_kernel(const uint4*, unsigned, float*);
extern "C" __global__ void bdpt_rand_planar_kernel(const float*, float*);
extern "C" __global__ void bdpt_sincos_planar_kernel(const float*, float2*);
extern "C" __global__ void bdpt_sample_records_kernel(const float*, float4*);
extern "C" __global__ void bdpt_light_kernel(const bdpt_dev_sphere*, unsigned, const float*, int,
                                             bdpt_dev_lightpath*);
extern "C" const void* bdpt_path_tiles_kernel_table[4];   // launches over a tile list: [(S > 1) * 2 + BVH]
extern "C" const void* bdpt_path_kernel_table[36];   // [(S > 1) * 18 + (BVH ? 17 : n <= 16 ? n : 0)]
extern "C" __global__ void bdpt_pixels_kernel(const bdpt_dev_vec*, uchar4*, const float*, int);
extern "C" __global__ void bdpt_accum_kernel(bdpt_path_args);
extern "C" __global__ void bdpt_accum_serial_kernel(bdpt_path_args);

extern "C" __global__ void bdpt_frame_add_kernel(float*, const float*, unsigned*, const unsigned*, int);

// gamma thresholds (host, once): see bdpt_util.c
extern "C" void bdpt_gamma_thresholds(float thr[256]);

static int upload_scene(bdpt_ctx* c) {
    c->tuner.reset();                                       // re-measure the stream mode
    jit_forget(c);                                          // the specialised kernels change too
    const unsigned n = (unsigned)c->spheres.size();
    // queued path passes may still read the scene buffers freed / rewritten below (pooled
    // launches on the pstreams: the last fold follows them all)
    if (int rc = join_fold(c)) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::vector<bdpt_dev_sphere> ds(n);
    std::vector<float4> geom(n), lrec;
    std::vector<float4> vgeom;                      // the non-emitters' geometry, ascending index
    c->lights.clear();
    c->emis_mask = 0;
    for (unsigned i = 0; i < n; i++) {
        const bdpt_sphere& s = c->spheres[i];
        bdpt_dev_sphere& d = ds[i];
        d.px = s.p.x; d.py = s.p.y; d.pz = s.p.z;
        d.rr = s.rad * s.rad;                       // the product SphereIntersectDevice forms
        d.ex = s.e.x; d.ey = s.e.y; d.ez = s.e.z;
        d.rad = s.rad;
        d.cx = s.c.x; d.cy = s.c.y; d.cz = s.c.z;
        d.refl = s.refl;
        geom[i] = make_float4(d.px, d.py, d.pz, d.rr);
        if (s.e.x == 0.f && s.e.y == 0.f && s.e.z == 0.f) vgeom.push_back(geom[i]);
        if (!(s.e.x == 0.f && s.e.y == 0.f && s.e.z == 0.f)) {
            c->lights.push_back((int)i);
            if (i < 32) c->emis_mask |= 1u << i;
            const float kPi = 3.14159265358979323846f;
            const float area = 4.f * kPi * s.rad * s.rad;        // device.cu:500, same float ops
            lrec.push_back(make_float4(s.p.x, s.p.y, s.p.z, s.rad));
            lrec.push_back(make_float4(s.e.x, s.e.y, s.e.z, area));
        }
    }
    if (n > c->sph_cap) {
        void* old[] = {c->d_sph, c->d_lights, c->d_geom, c->d_lightrec};
        for (void* b : old)
            if (b) HIPCHK(c, hipFree(b));
        c->d_sph = nullptr; c->d_lights = nullptr; c->d_geom = nullptr; c->d_lightrec = nullptr;
        HIPCHK(c, hipMalloc(&c->d_sph, sizeof(bdpt_dev_sphere) * n));
        HIPCHK(c, hipMalloc(&c->d_lights, sizeof(int) * n));
        HIPCHK(c, hipMalloc(&c->d_geom, 2 * sizeof(float4) * n));   // [n) by index, then the non-emitters
        HIPCHK(c, hipMalloc(&c->d_lightrec, 2 * sizeof(float4) * n));
        c->sph_cap = n;
    }
    if (n) HIPCHK(c, hipMemcpyAsync(c->d_geom, geom.data(), sizeof(float4) * n, hipMemcpyHostToDevice, c->stream));
    c->n_vac = (unsigned)vgeom.size();
    if (c->n_vac)
        HIPCHK(c, hipMemcpyAsync(c->d_geom + n, vgeom.data(), sizeof(float4) * c->n_vac, hipMemcpyHostToDevice,
                                 c->stream));
    if (!lrec.empty())
        HIPCHK(c, hipMemcpyAsync(c->d_lightrec, lrec.data(), sizeof(float4) * lrec.size(),
                                 hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_sph, ds.data(), sizeof(bdpt_dev_sphere) * n, hipMemcpyHostToDevice, c->stream));
    if (!c->lights.empty())
        HIPCHK(c, hipMemcpyAsync(c->d_lights, c->lights.data(), sizeof(int) * c->lights.size(),
                                 hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));

    // large scenes: BVH over the ordinary spheres + per-sphere material table in HBM
    void* old[] = {c->d_bvh_nodes, c->d_bvh_geom, c->d_big_geom, c->d_mat, c->d_bvh_ids, c->d_big_ids};
    for (void* b : old)
        if (b) HIPCHK(c, hipFree(b));
    c->d_bvh_nodes = c->d_bvh_geom = c->d_big_geom = c->d_mat = nullptr;
    c->d_bvh_ids = c->d_big_ids = nullptr;
    c->has_bvh = false;
    bdpt_bvh bvh;
    if (n > 16 && bdpt_build_bvh(c->spheres.data(), n, &bvh)) {
        std::vector<float4> mat(3 * (size_t)n);
        for (unsigned i = 0; i < n; i++) {
            const bdpt_dev_sphere& d = ds[i];
            const bool emis = !(d.ex == 0.f && d.ey == 0.f && d.ez == 0.f);
            mat[3 * i] = make_float4(d.cx, d.cy, d.cz, bdpt_bits_as_float(d.refl | (emis ? 256 : 0)));
            mat[3 * i + 1] = make_float4(d.ex, d.ey, d.ez, d.rad);
            mat[3 * i + 2] = make_float4(d.px, d.py, d.pz, 0.f);
        }
        c->bvh_nn = (int)bvh.nodes.size() / 2;
        c->bvh_ns = (int)bvh.geom.size();
        c->big_n = (int)bvh.big_geom.size();
        for (int k = 0; k < 3; k++) c->bvh_c[k] = bvh.c_root[k];
        c->bvh_r = bvh.r_root;
        c->bvh_q = bvh.q;
        HIPCHK(c, hipMalloc(&c->d_bvh_nodes, sizeof(float4) * bvh.nodes.size()));
        HIPCHK(c, hipMalloc(&c->d_bvh_geom, sizeof(float4) * bvh.geom.size()));
        HIPCHK(c, hipMalloc(&c->d_bvh_ids, sizeof(int) * bvh.ids.size()));
        HIPCHK(c, hipMalloc(&c->d_mat, sizeof(float4) * mat.size()));
        HIPCHK(c, hipMemcpy(c->d_bvh_nodes, bvh.nodes.data(), sizeof(float4) * bvh.nodes.size(), hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(c->d_bvh_geom, bvh.geom.data(), sizeof(float4) * bvh.geom.size(), hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(c->d_bvh_ids, bvh.ids.data(), sizeof(int) * bvh.ids.size(), hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(c->d_mat, mat.data(), sizeof(float4) * mat.size(), hipMemcpyHostToDevice));
        if (c->big_n) {
            HIPCHK(c, hipMalloc(&c->d_big_geom, sizeof(float4) * bvh.big_geom.size()));
            HIPCHK(c, hipMalloc(&c->d_big_ids, sizeof(int) * bvh.big_ids.size()));
            HIPCHK(c, hipMemcpy(c->d_big_geom, bvh.big_geom.data(), sizeof(float4) * bvh.big_geom.size(),
                                hipMemcpyHostToDevice));
            HIPCHK(c, hipMemcpy(c->d_big_ids, bvh.big_ids.data(), sizeof(int) * bvh.big_ids.size(),
                                hipMemcpyHostToDevice));
        }
        c->has_bvh = true;
    }
    return BDPT_OK;
}

static void release(bdpt_ctx* c) {
    void* bufs[] = {c->d_params, c->d_rand, c->d_rndp, c->d_scp, c->d_srec, c->d_lp, c->d_sph, c->d_lights, c->d_geom, c->d_lightrec, c->d_colors,
                    c->d_counter, c->d_pixels, c->d_thr, c->d_rbuf, c->d_rmask, c->d_poolctr, c->d_uflags, c->d_uerr, c->d_bvh_nodes,
                    c->d_bvh_geom, c->d_big_geom, c->d_mat, c->d_bvh_ids, c->d_big_ids,
                    c->d_fcolors, c->d_fcounter, c->d_fpixels, c->d_ftmp, c->d_ftmpc, c->d_aov, c->d_chain, c->d_dn, c->d_hist,
                    c->d_hdelta, c->d_mark, c->d_noise, c->d_tiles};
    for (void* b : bufs)
        if (b) (void)hipFree(b);
    for (const bdpt_svc_clock& k : c->svc)
        for (hipEvent_t e : k.ev)
            if (e) (void)hipEventDestroy(e);
    for (auto& s : c->ring) {
        for (hipEvent_t e : s.kev) (void)hipEventDestroy(e);
        if (s.ev0) (void)hipEventDestroy(s.ev0);
        if (s.ev1) (void)hipEventDestroy(s.ev1);
    }
    jit_release(c);
    for (int b = 0; b < 2; b++) {
        if (c->rb_path_ev[b]) (void)hipEventDestroy(c->rb_path_ev[b]);
        if (c->rb_fold_ev[b]) (void)hipEventDestroy(c->rb_fold_ev[b]);
    }
    if (c->amark) (void)hipEventDestroy(c->amark);
    for (hipStream_t& ps : c->pstream)
        if (ps) (void)hipStreamDestroy(ps);
    if (c->fstream) (void)hipStreamDestroy(c->fstream);
    if (c->stream) (void)hipStreamDestroy(c->stream);
}

// Passes per launch of the fused S = 1 kernel.  Its workgroups stage a VLP (48 B) and a sid per
// pass of the launch in LDS: 128 passes make 31.5 KB per workgroup.  Measured on caustic8 (one
// session, two rounds, profiles/r03_s1_ab_fused.txt): 64 passes at 5 waves/SIMD (4-KB sincos
// table) 48.8 Gs/s, 64 at 6 (2-KB table) 48.55, 128 at 6 48.2, 128 at 5 (round 2) 47.9.
// BDPT_FUSED_MAX_PASSES overrides.
int bdpt_host::fused_max_passes() {
    static const int cap = [] {
        const char* e = getenv("BDPT_FUSED_MAX_PASSES");
        const int v = e ? atoi(e) : 64;
        return v < 1 ? 1 : (v > 128 ? 128 : v);
    }();
    return cap;
}

// Pixel pools for the pass-stream kernel (bdpt_kernels.hip BDPT_POOL), a specialised build of
// its own launched with one pass per lane slice: the auto stream mode measures it (bdpt_plan.h).
// BDPT_POOL: unset = measured, 0 = never, R > 0 = always (streams launches), chunks of
// R x 64 pixels; BDPT_POOL_GRID = G: G x 64 pixels per wave and pass (bdpt_plan.h bdpt_pool_shape).
static int pool_env() {
    const char* e = getenv("BDPT_POOL");
    if (!e || !*e) return -1;
    const int v = atoi(e);
    return v < 1 ? 0 : (v > 64 ? 64 : v);
}

// Pass streams with the ordered fold inside the kernel (bdpt_kernels.hip BDPT_UNITS): BDPT_UNITS=P
// forces it with ranges of P passes (experiments; 0 = never).
int bdpt_host::units_env() {
    const char* e = getenv("BDPT_UNITS");
    if (!e || !*e) return -1;
    const int v = atoi(e);
    return v < 1 ? 0 : (v > 128 ? 128 : v);
}

// The planner's switches (bdpt_plan.h), read at every call -- tests and in-process A/Bs change
// them between calls -- except the three that are read once per process.
static bdpt_path_env path_env() {
    static const bdpt_path_env once = [] {
        bdpt_path_env e;
        e.fused_max_passes = fused_max_passes();
        if (const char* v = getenv("BDPT_POOL_OVERLAP")) e.pool_overlap = atoi(v) != 0;
        if (const char* v = getenv("BDPT_UNITS_TAPER")) e.units_taper = atoi(v) != 0;
        return e;
    }();
    bdpt_path_env e = once;
    e.pool = pool_env();
    e.units = units_env();
    if (const char* v = getenv("BDPT_MAX_LAUNCH_PASSES")) e.max_launch_passes = atoi(v);
    if (const char* v = getenv("BDPT_POOL_GRID")) e.pool_grid = std::min(atoi(v), 256);
    if (const char* v = getenv("BDPT_SMEM_PAD")) e.smem_pad = atoi(v);
    return e;
}

// Make the context's stream wait for the last pass-stream fold (issued on fstream): call before
// anything on `stream` touches colors/counter/pixels.  Folds run in order on fstream, so the last
// one covers all.
int bdpt_host::join_fold(bdpt_ctx* c) {
    if (c->cpu || !c->fold_pending) return BDPT_OK;
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->rb_fold_ev[c->fold_last], 0));
    c->fold_pending = false;
    return BDPT_OK;
}

// Fold the calls issued before call number `upto` into the accumulators, oldest first (waits
// for each of them to finish).
static int fold_timing(bdpt_ctx* c, long long upto) {
    for (; c->folded < upto && c->folded < c->issued; c->folded++) {
        bdpt_ctx::call_slot& s = c->ring[c->folded % bdpt_ctx::kRing];
        if (!s.pending) continue;
        float ms = 0.f;
        HIPCHK(c, hipEventSynchronize(s.ev1));
        HIPCHK(c, hipEventElapsedTime(&ms, s.ev0, s.ev1));
        c->last_ms = ms;
        c->acc_ms += ms;
        double kms = 0.0;
        for (int k = 0; k < s.launches; k++) {
            float km = 0.f;
            HIPCHK(c, hipEventElapsedTime(&km, s.kev[2 * k], s.kev[2 * k + 1]));
            kms += km;
        }
        c->acc_kernel_ms += kms;
        // the stream mode's measure: the path kernels' time plus a quarter of the rest of the
        // call (a pass-stream call's fold runs on its own stream beside the next call's path
        // kernels and costs about that much of its own time in back-to-back calls: caustic pools
        // 3.79 ms kernels + 1.10 ms fold -> 4.05 ms per call, two passes per lane 4.85 + 0.84 ->
        // 4.95, profiles/r04_s20_*)
        // (a call whose folds ran on its own stream after its path kernels is charged in full)
        for (int r = 0; r < kTuneRoles; r++)
            if (c->folded == c->tuner.call[r]) c->tuner.set_ms(r, s.serial_fold ? (double)ms : kms + 0.25 * ((double)ms - kms));
        c->acc_launches += s.launches;
        s.pending = false;
    }
    return BDPT_OK;
}
static int fold_timing(bdpt_ctx* c) { return fold_timing(c, c->issued); }

extern "C" {

const char* bdpt_last_error(const bdpt_ctx* c) { return c ? c->err : "null context"; }

static char g_create_err[512];

int bdpt_create(bdpt_ctx** out, const bdpt_sphere* spheres, unsigned n, int W, int H,
                const char* mt_dat_path, int device) {
    if (!out) return BDPT_EINVAL;
    *out = nullptr;
    bdpt_ctx* c = new (std::nothrow) bdpt_ctx();
    if (!c) return BDPT_ENOMEM;
    int rc = BDPT_OK;
    auto bail = [&](int code) {
        snprintf(g_create_err, sizeof(g_create_err), "%s", c->err);
        release(c);
        delete c;
        return code;
    };
    if (W <= 0 || H <= 0 || W > 65535 || H > 65535 || (long)W * (long)H > (1L << 30) || (n > 0 && !spheres))
        return (fail(c, BDPT_EINVAL, "bdpt_create: bad size %dx%d or spheres", W, H), bail(BDPT_EINVAL));
    c->W = W; c->H = H; c->device = device;
    c->spheres.assign(spheres, spheres + n);
    if (const char* e = getenv("BDPT_SPECIALIZE")) c->specialize = atoi(e) != 0;   // default for new contexts
    // loadMTGPU (MersenneTwister_kernel.cu:23-36): 4096 x 16 B records
    FILE* f = fopen(mt_dat_path ? mt_dat_path : "assets/data/MersenneTwister.dat", "rb");
    if (!f) return (fail(c, BDPT_EIO, "initMTGPU(): failed to open %s", mt_dat_path), bail(BDPT_EIO));
    size_t got = fread(c->h_params, sizeof(c->h_params), 1, f);
    fclose(f);
    if (got != 1) return (fail(c, BDPT_EIO, "initMTGPU(): failed to load %s", mt_dat_path), bail(BDPT_EIO));
    if (device == BDPT_DEVICE_CPU) {                          // the host backend: no HIP at all
        c->cpu = bdpt_cpu_create(spheres, n, W, H, c->h_params);
        if (!c->cpu) return (fail(c, BDPT_ENOMEM, "bdpt_create: CPU backend allocation"), bail(BDPT_ENOMEM));
        for (unsigned i = 0; i < n; i++)
            if (!(spheres[i].e.x == 0.f && spheres[i].e.y == 0.f && spheres[i].e.z == 0.f)) c->lights.push_back((int)i);
        c->specialize = false;
        *out = c;
        return BDPT_OK;
    }
    if (device < 0) return (fail(c, BDPT_EINVAL, "bdpt_create: bad device %d", device), bail(BDPT_EINVAL));

#define CK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { \
        fail(c, BDPT_EHIP, "%s: %s", #call, hipGetErrorString(e_)); return bail(BDPT_EHIP); } } while (0)
    CK(hipSetDevice(device));
    CK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    if (const char* tv = getenv("BDPT_STREAMS_TUNE")) c->tuner.enabled = atoi(tv) != 0;
    {
        // BDPT_FOLD_PRIORITY=high|low: the fold stream's priority (experiments; default normal)
        const char* fp = getenv("BDPT_FOLD_PRIORITY");
        int lo = 0, hi = 0;
        if (fp && hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess)
            CK(hipStreamCreateWithPriority(&c->fstream, hipStreamNonBlocking, !strcmp(fp, "high") ? hi : lo));
        else
            CK(hipStreamCreateWithFlags(&c->fstream, hipStreamNonBlocking));
    }
    for (int b = 0; b < 2; b++) {
        CK(hipEventCreateWithFlags(&c->rb_path_ev[b], hipEventDisableTiming));
        CK(hipEventCreateWithFlags(&c->rb_fold_ev[b], hipEventDisableTiming));
    }
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0)
            c->cus = cus;
        int lds = 0;
        CK(hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, device));
        c->lds_limit = (size_t)lds;
    }
    for (auto& s : c->ring) {
        CK(hipEventCreate(&s.ev0));
        CK(hipEventCreate(&s.ev1));
    }
    const size_t np = (size_t)W * H;
    CK(hipMalloc(&c->d_params, sizeof(c->h_params)));
    CK(hipMalloc(&c->d_rand, sizeof(float) * BDPT_RAND_N));
    CK(hipMalloc(&c->d_rndp, sizeof(float) * BDPT_DEV_RANDP_PLANES * BDPT_DEV_RANDP_PL));
    CK(hipMalloc(&c->d_lp, sizeof(bdpt_dev_lightpath) * BDPT_LIGHT_POINTS));
    CK(hipMalloc(&c->d_colors, sizeof(bdpt_dev_vec) * np));
    CK(hipMalloc(&c->d_counter, sizeof(unsigned) * np));
    CK(hipMalloc(&c->d_pixels, sizeof(uchar4) * np));
    CK(hipMalloc(&c->d_thr, sizeof(float) * 256));
    CK(hipMemsetAsync(c->d_lp, 0, sizeof(bdpt_dev_lightpath) * BDPT_LIGHT_POINTS, c->stream));
    CK(hipMemsetAsync(c->d_colors, 0, sizeof(bdpt_dev_vec) * np, c->stream));
    CK(hipMemsetAsync(c->d_counter, 0, sizeof(unsigned) * np, c->stream));
    CK(hipMemsetAsync(c->d_pixels, 0, sizeof(uchar4) * np, c->stream));
    float thr[256];
    bdpt_gamma_thresholds(thr);
    CK(hipMemcpyAsync(c->d_thr, thr, sizeof(thr), hipMemcpyHostToDevice, c->stream));
    CK(hipStreamSynchronize(c->stream));
#undef CK
    rc = upload_scene(c);
    if (rc != BDPT_OK) return bail(rc);
    *out = c;
    return BDPT_OK;
}

const char* bdpt_create_error(void) { return g_create_err; }

static void destroy_group(bdpt_ctx* c);

void bdpt_destroy(bdpt_ctx* c) {
    if (!c) return;
    if (c->cpu) {
        bdpt_cpu_destroy(c->cpu);
        delete c;
        return;
    }
    destroy_group(c);
    (void)hipSetDevice(c->device);
    if (c->fstream) (void)hipStreamSynchronize(c->fstream);
    for (hipStream_t ps : c->pstream)
        if (ps) (void)hipStreamSynchronize(ps);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->d_prof) {                 // section profile of a -DBDPT_PROF kernel (experiments)
        unsigned long long p[24] = {};
        const char* pe = getenv("BDPT_PROF");
        if (pe && !strcmp(pe, "counts") && hipMemcpy(p, c->d_prof, sizeof p, hipMemcpyDeviceToHost) == hipSuccess) {
            fprintf(stderr, "bdpt_counts");        // region counts of a -DBDPT_COUNTS kernel
            for (int q = 0; q < 24; q++) fprintf(stderr, " %llu", p[q]);
            fprintf(stderr, "\n");
        } else if (hipMemcpy(p, c->d_prof, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost) == hipSuccess) {
            double tot = 0;
            for (int q = 0; q < 6; q++) tot += (double)p[q];
            fprintf(stderr, "bdpt_prof waves=%llu cycles/wave=%.0f", p[7], p[7] ? tot / p[7] : 0.0);
            for (int q = 0; q < 6; q++) fprintf(stderr, " s%d=%.4f", q, tot > 0 ? p[q] / tot : 0.0);
            fprintf(stderr, "\n");
        }
        (void)hipFree(c->d_prof);
    }
    if (c->gl_res) (void)hipGraphicsUnregisterResource(c->gl_res);
    release(c);
    delete c;
}

// (set_scene, set_camera, reset_accum and write_radiance rewrite the accumulation or what it is
// an accumulation of: they clear the noise estimate's mark -- a flag here, the CPU backend's own)
static int one_set_scene(bdpt_ctx* c, const bdpt_sphere* spheres, unsigned n) {
    if (!c || (n > 0 && !spheres)) return BDPT_EINVAL;
    c->mark_live = false;
    if (c->cpu) {
        c->spheres.assign(spheres, spheres + n);
        bdpt_cpu_set_scene(c->cpu, spheres, n);
        return BDPT_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    c->spheres.assign(spheres, spheres + n);
    return upload_scene(c);
}

static int one_set_camera(bdpt_ctx* c, const bdpt_camera* cam) {
    if (!c || !cam) return BDPT_EINVAL;
    c->mark_live = false;
    if (c->cpu) bdpt_cpu_set_camera(c->cpu, cam);
    c->cam = *cam;
    c->cam_set = true;
    return BDPT_OK;
}

static int one_reset_accum(bdpt_ctx* c) {
    if (!c) return BDPT_EINVAL;
    c->mark_live = false;
    if (c->cpu) {
        bdpt_cpu_reset_accum(c->cpu);
        return BDPT_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = join_fold(c)) return rc;
    HIPCHK(c, hipMemsetAsync(c->d_counter, 0, sizeof(unsigned) * (size_t)c->W * c->H, c->stream));
    if (c->d_uerr) {                                         // a new frame: no stale handover error
        HIPCHK(c, hipMemsetAsync(c->d_uerr, 0, sizeof(unsigned), c->stream));
        c->units_check = false;
    }
    return BDPT_OK;
}

static int one_set_shard(bdpt_ctx* c, int shard, int nshards, int band_rows) {
    if (!c || nshards < 1 || shard < 0 || shard >= nshards || band_rows < 1)
        return c ? fail(c, BDPT_EINVAL, "bdpt_set_shard: bad shard %d/%d band %d", shard, nshards, band_rows)
                 : BDPT_EINVAL;
    c->shard = shard; c->nshards = nshards; c->band_rows = band_rows;
    c->tuner.reset();
    if (c->cpu) bdpt_cpu_set_shard(c->cpu, shard, nshards, band_rows);
    return BDPT_OK;
}

static int one_set_streams(bdpt_ctx* c, int streams) {
    if (!c) return BDPT_EINVAL;
    if (streams < BDPT_STREAMS_PER_LANE || streams > BDPT_MAX_STREAMS)
        return fail(c, BDPT_EINVAL, "bdpt_set_streams: bad stream count %d", streams);
    c->streams_req = streams;
    c->tuner.reset();
    return BDPT_OK;
}

int bdpt_last_streams(const bdpt_ctx* c) { return c ? c->last_streams : BDPT_EINVAL; }

static int choice_of(const bdpt_ctx* c) {
    return c->streams_req == 0 ? c->tuner.choice() : 0;
}

static int one_set_stream_choice(bdpt_ctx* c, int choice) {
    if (!c) return BDPT_EINVAL;
    if (!(choice & BDPT_CHOICE_DECIDED) || (choice & ~0x3f) ||
        ((choice & BDPT_CHOICE_POOLS) && (choice & BDPT_CHOICE_UNITS)))
        return fail(c, BDPT_EINVAL, "bdpt_set_stream_choice: bad choice 0x%x", choice);
    if (c->streams_req != 0)
        return fail(c, BDPT_ESTATE, "bdpt_set_stream_choice: the stream mode is not auto (%d)", c->streams_req);
    c->tuner.set_choice(choice);
    return BDPT_OK;
}

int bdpt_stream_choice(const bdpt_ctx* c) { return c ? choice_of(c) : BDPT_EINVAL; }

static int one_set_specialize(bdpt_ctx* c, int on) {
    if (!c) return BDPT_EINVAL;
    c->specialize = on != 0;
    jit_forget(c);
    c->tuner.reset();
    return BDPT_OK;
}

int bdpt_last_specialized(const bdpt_ctx* c) { return c ? (int)c->last_specialized : BDPT_EINVAL; }

const char* bdpt_specialize_status(const bdpt_ctx* c) { return c ? c->jit_err : "null context"; }

static int one_set_traversal(bdpt_ctx* c, int mode) {
    if (!c) return BDPT_EINVAL;
    if (mode != BDPT_TRAVERSE_AUTO && mode != BDPT_TRAVERSE_BRUTE && mode != BDPT_TRAVERSE_BVH)
        return fail(c, BDPT_EINVAL, "bdpt_set_traversal: bad mode %d", mode);
    c->traversal = mode;
    c->tuner.reset();
    return BDPT_OK;
}

int bdpt_scene_has_bvh(const bdpt_ctx* c) { return c ? (int)c->has_bvh : BDPT_EINVAL; }

int bdpt_last_traversal(const bdpt_ctx* c) {
    return c ? (c->last_bvh ? BDPT_TRAVERSE_BVH : BDPT_TRAVERSE_BRUTE) : BDPT_EINVAL;
}

static int one_generate_rand(bdpt_ctx* c, unsigned seed) {
    if (!c) return BDPT_EINVAL;
    if (c->cpu) {
        bdpt_cpu_generate_rand(c->cpu, seed);
        c->rand_ready = true;
        c->rand_seed = seed;
    c->rand_uploaded = false;
        return BDPT_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = join_fold(c)) return rc;              // path kernels read the table
    // seedMTGPU(seed): every record's seed field := seed (MersenneTwister_kernel.cu:44-47)
    std::vector<uint32_t> p(c->h_params, c->h_params + 4 * BDPT_MT_RNG_COUNT);
    for (int i = 0; i < BDPT_MT_RNG_COUNT; i++) p[4 * i + 3] = seed;
    HIPCHK(c, hipMemcpyAsync(c->d_params, p.data(), sizeof(uint32_t) * p.size(), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(bdpt_mt607_kernel, dim3(BDPT_MT_RNG_COUNT / 64), dim3(64), 0, c->stream,
                       (const uint4*)c->d_params, seed, c->d_rand);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(bdpt_rand_planar_kernel, dim3((BDPT_DEV_RANDP_PLANES * BDPT_DEV_RANDP_PL + 255) / 256),
                       dim3(256), 0, c->stream, (const float*)c->d_rand, c->d_rndp);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->rand_ready = true;
    c->scp_ready = c->srec_ready = false;              // rebuilt by the next launch that reads them
    c->rand_seed = seed;
    c->rand_uploaded = false;
    return BDPT_OK;
}

// The derived tables, built on the context's stream (the path kernels that read them run on it)
// from the current d_rand / d_rndp; no-ops while they are current.
static int ensure_scp(bdpt_ctx* c) {
    if (c->scp_ready) return BDPT_OK;
    const size_t n = (size_t)BDPT_DEV_RANDP_PLANES * BDPT_DEV_RANDP_PL;
    if (!c->d_scp && hipMalloc(&c->d_scp, sizeof(float2) * n) != hipSuccess) {
        (void)hipGetLastError();
        c->d_scp = nullptr;
        return fail(c, BDPT_ENOMEM, "sin/cos planes (%zu B)", sizeof(float2) * n);
    }
    hipLaunchKernelGGL(bdpt_sincos_planar_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream,
                       (const float*)c->d_rndp, c->d_scp);
    HIPCHK(c, hipGetLastError());
    c->scp_ready = true;
    return BDPT_OK;
}

static int ensure_srec(bdpt_ctx* c) {
    if (c->srec_ready) return BDPT_OK;
    const size_t n = 2 * (size_t)BDPT_DEV_SREC_HALF;
    if (!c->d_srec && hipMalloc(&c->d_srec, sizeof(float4) * n) != hipSuccess) {
        (void)hipGetLastError();
        c->d_srec = nullptr;
        return fail(c, BDPT_ENOMEM, "sample records (%zu B)", sizeof(float4) * n);
    }
    hipLaunchKernelGGL(bdpt_sample_records_kernel, dim3((BDPT_DEV_SREC_HALF + 255) / 256), dim3(256), 0, c->stream,
                       (const float*)c->d_rand, c->d_srec);
    HIPCHK(c, hipGetLastError());
    c->srec_ready = true;
    return BDPT_OK;
}

static int one_light_pass(bdpt_ctx* c, int current_sample) {
    if (!c) return BDPT_EINVAL;
    if (c->cpu) {
        bdpt_cpu_light_pass(c->cpu, current_sample);
        c->rand_ready = true;
        c->rand_seed = (unsigned)(current_sample * 5);
        c->rand_uploaded = false;
        return BDPT_OK;
    }
    // The reference regenerates the table per light with the same seed (smallpt_cpu.c:321-322):
    // one generation is identical.  With no emitter it launches nothing and the path pass reads
    // an uninitialised d_Rand; we generate the table anyway (the frame is black either way:
    // there is no emission, and dev_lp stays zero) so the run is defined.
    int rc = one_generate_rand(c, (unsigned)(current_sample * 5));
    if (rc) return rc;
    if (c->lights.empty()) return BDPT_OK;
    hipLaunchKernelGGL(bdpt_light_kernel, dim3(BDPT_LIGHT_POINTS / 64), dim3(64), 0, c->stream,
                       (const bdpt_dev_sphere*)c->d_sph, (unsigned)c->spheres.size(),
                       (const float*)c->d_rand, current_sample, c->d_lp);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BDPT_OK;
}

// The frame and camera constants of a launch (the by-value Camera of device.cu:548, as the kernels
// take it): shared by the path passes and the frame kernels.  The terms are bdpt_eye.h's, the one
// statement of them, which the CPU backend uses too.
extern "C++" void bdpt_host::camera_args(const bdpt_ctx* c, const bdpt_camera& cam, bdpt_path_args& a) {
    const eye_camera e = eye_camera_terms(cam, c->W, c->H);
    static_assert(sizeof(f3) == sizeof(a.ux), "f3 is three packed floats");
    a.W = c->W; a.H = c->H;
    a.inv_w = e.inv_w; a.inv_h = e.inv_h; a.half_w = e.half_w; a.half_h = e.half_h;
    memcpy(a.ux, &e.ux, sizeof(a.ux)); memcpy(a.uy, &e.uy, sizeof(a.uy)); memcpy(a.ud, &e.ud, sizeof(a.ud));
    memcpy(a.orig, &e.orig, sizeof(a.orig));
    a.tx = e.tx; a.ty = e.ty; a.tz = e.tz;
}
static void camera_args(const bdpt_ctx* c, bdpt_path_args& a) { camera_args(c, c->cam, a); }

// ---- bdpt_path_passes: the steps of one call, in the order one_path_passes runs them.  What a
// call launches is decided in bdpt_plan.h; the functions below issue it. ----

static int cpu_path_passes(bdpt_ctx* c, const unsigned* sid, const int* vlp, int npass, const unsigned char* mask) {
    const auto t0 = std::chrono::steady_clock::now();       // synchronous; wall-clock timing
    bdpt_cpu_path_passes(c->cpu, sid, vlp, npass, mask);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    c->last_ms = (float)ms;
    c->acc_ms += ms;
    c->acc_kernel_ms += ms;
    c->acc_launches += 1;
    c->last_streams = 1;
    c->last_specialized = false;
    c->last_bvh = false;
    c->last_features = mask ? BDPT_FEAT_TILES : 0;
    return BDPT_OK;
}

// The argument fields every launch of the context shares, whatever the plan.
static int path_args_base(bdpt_ctx* c, bdpt_path_args& a) {
    memset(&a, 0, sizeof(a));
    a.sph = c->d_sph;
    a.n = (unsigned)c->spheres.size();
    a.n_lights = (unsigned)c->lights.size();
    a.lights = c->d_lights;
    a.lightrec = c->d_lightrec;
    a.geom = c->d_geom;
    a.vgeom = c->d_geom + c->spheres.size();
    a.n_vac = (int)c->n_vac;
    a.emis_mask = c->emis_mask;
    a.rnd = c->d_rand;
    a.rndp = c->d_rndp;
    a.lp = c->d_lp;
    a.colors = c->d_colors;
    a.counter = c->d_counter;
    a.pixels = c->d_pixels;
    a.gamma_thr = c->d_thr;
    camera_args(c, a);
    a.shard = c->shard; a.nshards = c->nshards; a.band_rows = c->band_rows;
    if (!c->d_prof && getenv("BDPT_PROF")) {
        HIPCHK(c, hipMalloc(&c->d_prof, 24 * sizeof(unsigned long long)));
        HIPCHK(c, hipMemset(c->d_prof, 0, 24 * sizeof(unsigned long long)));
    }
    a.prof = c->d_prof;
    return BDPT_OK;
}

// The BVH fields of a launch that traverses it: the path passes' (path_args_plan) and the
// feature-buffer kernel's (bdpt_frame.cpp aov_launch).
extern "C++" void bdpt_host::bvh_args(const bdpt_ctx* c, bdpt_path_args& a) {
    a.bvh_nodes = c->d_bvh_nodes; a.bvh_geom = c->d_bvh_geom; a.bvh_ids = c->d_bvh_ids;
    a.big_geom = c->d_big_geom; a.big_ids = c->d_big_ids;
    a.bvh_nn = c->bvh_nn; a.bvh_ns = c->bvh_ns; a.big_n = c->big_n;
    for (int k = 0; k < 3; k++) a.bvh_c[k] = c->bvh_c[k];
    a.bvh_r = c->bvh_r;
    a.bvh_q = c->bvh_q;
}

// The plan's part of the arguments: the shard's grid and, for a plan that traverses it, the BVH.
static void path_args_plan(const bdpt_ctx* c, const bdpt_plan& plan, bdpt_path_args& a) {
    a.tiles_per_band = plan.tiles_per_band;
    a.nloc = (int)plan.lanes;
    a.gx = plan.gx;
    a.gy = plan.grid_rows;
    if (!plan.bvh) return;
    bvh_args(c, a);
    a.mat = c->d_mat;
}

// Auto stream mode with every role's call issued: a group peer takes the decision of devices[0]
// once that exists; otherwise wait for the last measured call and decide.
static int settle_stream_mode(bdpt_ctx* c) {
    bdpt_tuner& t = c->tuner;
    if (c->streams_req != 0 || !t.enabled || t.measuring() || t.decided()) return BDPT_OK;
    const bdpt_ctx* lead = c->group_leader;
    if (lead && lead->streams_req == 0 && lead->tuner.decided()) {
        t.adopt(lead->tuner);
        return BDPT_OK;
    }
    if (int rc = fold_timing(c, t.call[kTuneRoles - 1] + 1)) return rc;
    t.decide();
    return BDPT_OK;
}

// The pass-stream radiance buffer and the pools' mask (two halves each), grown to the plan's
// largest launch; the in-kernel fold needs neither.  `units`: the units build resolved -- a plan
// that wants units without it (specialisation off, or a build that failed) launches the plain
// pass-stream kernel, which writes the buffer.
static int ensure_radiance_buffers(bdpt_ctx* c, const bdpt_plan& plan, int npass, bool units) {
    if (plan.S <= 1 || units) return BDPT_OK;
    const size_t lanes = (size_t)plan.lanes;
    const size_t need = (size_t)(npass < plan.chunk ? npass : plan.chunk) * lanes;
    if (need <= c->rbuf_cap && lanes <= c->rmask_lanes) return BDPT_OK;
    HIPCHK(c, hipStreamSynchronize(c->stream));             // queued passes and folds may use it
    HIPCHK(c, hipStreamSynchronize(c->fstream));
    for (hipStream_t ps : c->pstream)
        if (ps) HIPCHK(c, hipStreamSynchronize(ps));
    if (c->d_rbuf) HIPCHK(c, hipFree(c->d_rbuf));
    if (c->d_rmask) HIPCHK(c, hipFree(c->d_rmask));
    c->d_rbuf = nullptr;
    c->d_rmask = nullptr;
    c->rbuf_cap = 0;
    c->rb_used[0] = c->rb_used[1] = false;
    if (hipMalloc(&c->d_rbuf, 2 * sizeof(bdpt_dev_vec) * need) != hipSuccess)
        return fail(c, BDPT_ENOMEM, "bdpt_path_passes: pass-stream buffer (2 x %zu B)", sizeof(bdpt_dev_vec) * need);
    if (hipMalloc(&c->d_rmask, 2 * 16 * lanes) != hipSuccess)
        return fail(c, BDPT_ENOMEM, "bdpt_path_passes: pass-stream mask (2 x %zu B)", 16 * lanes);
    c->rmask_lanes = lanes;
    c->rbuf_cap = need;
    // touch every page now (queued before this call's timing event): the first launch
    // would otherwise pay the first-touch cost, and the stream-mode measurement with it
    HIPCHK(c, hipMemsetAsync(c->d_rbuf, 0, 2 * sizeof(bdpt_dev_vec) * need, c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_rmask, 0, 2 * 16 * lanes, c->stream));
    return BDPT_OK;
}

// The specialised kernels of a call by bdpt_launch_kernel (nullptr: the precompiled instance runs),
// and what its launches need besides.
struct path_kernels {
    hipFunction_t jf[BDPT_KERNEL_KINDS] = {};
    bool any_fused = false, any_streams = false;
    bool use_srec = false;          // the pass-stream launches read sample records
};

// Resolve the specialised kernels (a compile on first use) and build the derived table the call's
// pass-stream kernels read, both before the timed region starts.
static int resolve_path_kernels(bdpt_ctx* c, const bdpt_plan& plan, int npass, bdpt_path_args& a, path_kernels& k) {
    // a kind's variant for this call: over the call's tile list if it has one (a masked call never
    // wants pools or units, bdpt_plan.h), the fused kernel with the planned pairing
    auto variant = [&plan](int kind) {
        bdpt_jit_variant v;
        v.kind = kind;
        v.pair = kind == BDPT_KERNEL_FUSED ? plan.pair : true;
        v.tiles = plan.ntiles >= 0;
        return v;
    };
    for (int p0 = 0; plan.launches > 0 && p0 < npass; p0 += plan.chunk) {
        const int np = npass - p0 < plan.chunk ? npass - p0 : plan.chunk;
        const bool st = (plan.S < np ? plan.S : np) > 1;
        k.any_fused |= !st;
        k.any_streams |= st;
        if (plan.bvh) continue;
        hipFunction_t& pool = k.jf[BDPT_KERNEL_POOL], &units = k.jf[BDPT_KERNEL_UNITS];
        if (st && plan.want_pool && !pool) pool = jit_path_kernel(c, variant(BDPT_KERNEL_POOL));
        if (st && plan.want_units && !units) units = jit_path_kernel(c, variant(BDPT_KERNEL_UNITS));
        if (st && !pool && !units && !k.jf[BDPT_KERNEL_STREAMS])
            k.jf[BDPT_KERNEL_STREAMS] = jit_path_kernel(c, variant(BDPT_KERNEL_STREAMS));
        if (!st && !k.jf[BDPT_KERNEL_FUSED]) k.jf[BDPT_KERNEL_FUSED] = jit_path_kernel(c, variant(BDPT_KERNEL_FUSED));
    }
    // the derived table (the pooled build reads neither): sample records for a specialised build
    // that has them, else the sin/cos planes -- built if the table changed since they last were
    const bool pool = k.jf[BDPT_KERNEL_POOL] != nullptr;
    k.use_srec = k.any_streams && !pool && (k.jf[BDPT_KERNEL_UNITS] || k.jf[BDPT_KERNEL_STREAMS]) && jit_srec_enabled();
    const bool use_scp = k.any_streams && !pool && !k.use_srec;
    if (k.use_srec)
        if (int rc = ensure_srec(c)) return rc;
    if (use_scp)
        if (int rc = ensure_scp(c)) return rc;
    a.scp = k.use_srec ? (const float2*)c->d_srec : use_scp ? c->d_scp : nullptr;
    return BDPT_OK;
}

// The LDS table terms of the call's launches (bdpt_plan.h bdpt_path_smem): scene tables (4 per
// sphere + the non-emitters, or the BVH's brute-force spheres) and those spheres' ids.
static void path_lds_table(const bdpt_path_args& a, bool bvh, size_t* tab, size_t* ids) {
    *tab = bdpt_path_tab(bvh, a.n, (size_t)a.n_vac, (size_t)a.big_n);
    *ids = bvh ? a.big_n : 0;
}

// The precompiled instance of a launch: by sphere count (or the BVH's), or for a launch over a tile
// list the generic instance (any sphere count) or the BVH's with the tile-list code.
static const void* precompiled_path_kernel(const bdpt_plan& plan, const bdpt_launch& L) {
    return plan.ntiles >= 0 ? bdpt_path_tiles_kernel_table[L.st * 2 + plan.bvh] : bdpt_path_kernel_table[L.st * 18 + plan.kidx];
}

// Static LDS of the function a launch runs (HIP_FUNC_ATTRIBUTE_SHARED_SIZE_BYTES: the camera basis,
// the sincos table, the claim words), asked once per function.
static int path_kernel_static_lds(bdpt_ctx* c, const bdpt_plan& plan, const bdpt_launch& L, const path_kernels& k,
                                  size_t* stat) {
    const hipFunction_t jf = k.jf[L.kernel];
    const void* key = jf ? (const void*)jf : precompiled_path_kernel(plan, L);
    for (const auto& e : c->lds_static)
        if (e.first == key) {
            *stat = e.second;
            return BDPT_OK;
        }
    if (jf) {
        int v = 0;
        HIPCHK(c, hipFuncGetAttribute(&v, HIP_FUNC_ATTRIBUTE_SHARED_SIZE_BYTES, jf));
        *stat = (size_t)v;
    } else {
        hipFuncAttributes at;
        HIPCHK(c, hipFuncGetAttributes(&at, key));
        *stat = at.sharedSizeBytes;
    }
    c->lds_static.emplace_back(key, *stat);
    return BDPT_OK;
}

// Every launch of the call must fit the device's LDS per workgroup, static part included
// (bdpt_plan.h bdpt_path_lds_fits): checked for all of them before anything of the call is issued.
static int check_path_lds(bdpt_ctx* c, const bdpt_plan& plan, const path_kernels& k, size_t tab, size_t ids,
                          const bdpt_path_env& env, int npass, unsigned n) {
    c->last_lds_static = c->last_lds_dynamic = 0;
    int launches = 0;
    for (int p0 = 0; launches < plan.launches; p0 += plan.chunk, launches++) {
        const bdpt_launch L = bdpt_plan_launch(plan, p0, npass, k.jf[BDPT_KERNEL_POOL] != nullptr,
                                               k.jf[BDPT_KERNEL_UNITS] != nullptr, k.jf[BDPT_KERNEL_STREAMS] != nullptr,
                                               k.jf[BDPT_KERNEL_FUSED] != nullptr, k.use_srec, c->jit_zero_exit, tab, ids, env);
        size_t stat = 0;
        if (int rc = path_kernel_static_lds(c, plan, L, k, &stat)) return rc;
        if (L.smem + stat > c->last_lds_static + c->last_lds_dynamic) {
            c->last_lds_static = stat;
            c->last_lds_dynamic = L.smem;
        }
    }
    if (!bdpt_path_lds_fits(c->last_lds_dynamic, c->last_lds_static, c->lds_limit))
        return fail(c, BDPT_EINVAL, "bdpt_path_passes: scene too large for LDS (%u spheres)", n);
    return BDPT_OK;
}

// A call between begin_call and end_call.
struct path_call {
    bdpt_ctx::call_slot* cs = nullptr;
    // Pixel pools fold on the launch's stream right after each path kernel (serial fold, over
    // their sparse radiance): the concurrent fold's HBM traffic slowed the next call's pooled path
    // kernel more than the fold costs on its own -- caustic pools 4.10 -> 4.04-4.07 ms per call,
    // path kernel 3.93 -> 3.29-3.31 ms; two passes per lane keep the concurrent fold (cornell
    // S = 64 33.82 -> 33.92 ms serial), profiles/r05_s11_serial_fold.txt.
    bool serial_fold = false;
    bool overlap = false;           // pooled launches on the pstreams (bdpt_plan.h bdpt_plan_overlap)
    bool ev0_done = false;
    int launches = 0;
    bool pool_ran = false, units_ran = false;
};

// Order the call behind the outstanding fold where it must be, and start its timing.
static int begin_call(bdpt_ctx* c, const bdpt_plan& plan, const bdpt_path_env& env, const path_kernels& k,
                      path_call& call) {
    call.serial_fold = k.jf[BDPT_KERNEL_POOL] != nullptr;
    call.overlap = bdpt_plan_overlap(plan, env, call.serial_fold);
    // a fused launch updates colors itself, and a serial fold does so on this stream: they wait
    // for the outstanding concurrent fold, before the call's timing starts (so the stream-mode
    // measurement does not charge that fold to it); overlapped pooled launches order their folds
    // through rb_fold_ev instead
    if (k.any_fused || k.jf[BDPT_KERNEL_UNITS] || (call.serial_fold && !call.overlap))
        if (int rc = join_fold(c)) return rc;
    if (call.overlap) {
        if (!c->pstream[0]) {
            for (hipStream_t& ps : c->pstream) HIPCHK(c, hipStreamCreateWithFlags(&ps, hipStreamNonBlocking));
            HIPCHK(c, hipEventCreateWithFlags(&c->amark, hipEventDisableTiming));
        }
        HIPCHK(c, hipEventRecord(c->amark, c->stream));  // the pstreams follow `stream`'s earlier work
    }
    call.ev0_done = !call.overlap;                       // (overlapped: the first launch's stream starts it)
    if (!call.overlap) HIPCHK(c, hipEventRecord(call.cs->ev0, c->stream));
    return BDPT_OK;
}

// Pixel pools (a specialised pass-stream build with BDPT_POOL): the chunk size and the launch's
// claim counters, per pass 8 of them, a 128-B line each.
static int prepare_pool_launch(bdpt_ctx* c, const bdpt_launch& L, hipStream_t ls, int half, bdpt_path_args& a) {
    if (L.streams != L.npass || L.npass > 128)
        return fail(c, BDPT_EINVAL, "bdpt_path_passes: pixel pools need one pass per stream (%d of %d)",
                    L.streams, L.npass);
    constexpr size_t kSet = 128 * 8 * 32;                // words per set
    if (!c->d_poolctr) {
        HIPCHK(c, hipMalloc(&c->d_poolctr, 2 * kSet * sizeof(unsigned)));
        HIPCHK(c, hipMemsetAsync(c->d_poolctr, 0, 2 * kSet * sizeof(unsigned), c->stream));
        c->pool_set = 0;
    }
    a.pool = L.pool;
    if (L.overlap) {
        // set `half`, cleared on this launch's stream (its previous user, the launch two
        // back, ran earlier on the same stream); the kernel clears no next set
        a.pool_ctr = c->d_poolctr + (size_t)half * kSet;
        a.pool_ctr_next = nullptr;
        HIPCHK(c, hipMemsetAsync(a.pool_ctr, 0, kSet * sizeof(unsigned), ls));
        c->pool_dirty = true;
    } else {
        if (c->pool_dirty) {                             // overlapped launches left both sets used
            HIPCHK(c, hipMemsetAsync(c->d_poolctr, 0, 2 * kSet * sizeof(unsigned), c->stream));
            c->pool_dirty = false;
        }
        a.pool_ctr = c->d_poolctr + (size_t)c->pool_set * kSet;
        a.pool_ctr_next = c->d_poolctr + (size_t)(c->pool_set ^ 1) * kSet;
        c->pool_set ^= 1;
    }
    return BDPT_OK;
}

// The ordered in-kernel fold: one workgroup per unit, each claims its unit from its XCD's queue
// (bdpt_kernels.hip); the queue counters, the tiles' flags and this launch's tag.
static int prepare_units_launch(bdpt_ctx* c, const bdpt_plan& plan, const bdpt_launch& L, bdpt_path_args& a) {
    const int wgs = plan.gx * plan.grid_rows;
    a.unit_taper = L.unit_taper;
    const size_t nflags = (size_t)wgs * 4;
    if (!c->d_uerr) {                                    // error word + 8 queue counters, 128 B apart
        HIPCHK(c, hipMalloc(&c->d_uerr, sizeof(unsigned) * (32 + 8 * 32)));
        HIPCHK(c, hipMemsetAsync(c->d_uerr, 0, sizeof(unsigned), c->stream));
    }
    HIPCHK(c, hipMemsetAsync(c->d_uerr + 32, 0, sizeof(unsigned) * 8 * 32, c->stream));
    if (nflags > c->uflags_cap || ((c->uepoch + 1) & 0xffffffu) == 0) {
        if (nflags > c->uflags_cap) {
            HIPCHK(c, hipStreamSynchronize(c->stream));
            if (c->d_uflags) HIPCHK(c, hipFree(c->d_uflags));
            c->d_uflags = nullptr;
            HIPCHK(c, hipMalloc(&c->d_uflags, sizeof(unsigned) * nflags));
            c->uflags_cap = nflags;
        }
        HIPCHK(c, hipMemsetAsync(c->d_uflags, 0, sizeof(unsigned) * c->uflags_cap, c->stream));
        c->uepoch = 0;
    }
    c->uepoch++;                                         // tags never repeat within 2^24 launches
    a.unit_tag = c->uepoch << 8;
    a.unit_flags = c->d_uflags;
    a.unit_err = c->d_uerr;
    a.unit_ctr = c->d_uerr + 32;
    a.unit_wgs = wgs;
    a.gx = plan.gx;
    a.gy = plan.grid_rows;
    c->units_check = true;
    return BDPT_OK;
}

// The fold of a pass-stream launch's radiance half into colors (1-D over the launch's rows):
// after the path kernel on its stream (pools), or on fstream beside the next path kernel.
static int issue_fold(bdpt_ctx* c, const path_call& call, long lanes, hipStream_t ls, int half, void** kargs) {
    const dim3 fgrid((unsigned)((lanes + 255) / 256), 1, 1), block(256);
    if (call.serial_fold) {
        // (overlapped: after the previous fold too, wherever it ran)
        if (call.overlap && c->fold_pending) HIPCHK(c, hipStreamWaitEvent(ls, c->rb_fold_ev[c->fold_last], 0));
        HIPCHK(c, hipLaunchKernel((const void*)&bdpt_accum_serial_kernel, fgrid, block, kargs, 0, ls));
        if (!call.overlap) return BDPT_OK;
        HIPCHK(c, hipEventRecord(c->rb_fold_ev[half], ls));
        c->fold_stream = ls;
    } else {                                             // the ordered fold, on fstream
        HIPCHK(c, hipEventRecord(c->rb_path_ev[half], c->stream));
        HIPCHK(c, hipStreamWaitEvent(c->fstream, c->rb_path_ev[half], 0));
        // after the previous fold (an overlapped pooled launch's ran on a pstream)
        if (c->fold_pending && c->fold_stream != c->fstream)
            HIPCHK(c, hipStreamWaitEvent(c->fstream, c->rb_fold_ev[c->fold_last], 0));
        c->fold_stream = c->fstream;
        HIPCHK(c, hipLaunchKernel((const void*)&bdpt_accum_kernel, fgrid, block, kargs, 0, c->fstream));
        HIPCHK(c, hipEventRecord(c->rb_fold_ev[half], c->fstream));
    }
    c->rb_used[half] = true;
    c->fold_last = half;
    c->fold_pending = true;
    c->rb_next = half ^ 1;
    return BDPT_OK;
}

// One launch: its pass table and mode fields, its radiance half, the path kernel between the
// launch's two timing events, and its fold.
static int launch_path_kernel(bdpt_ctx* c, const bdpt_plan& plan, const bdpt_launch& L, const path_kernels& k,
                              path_call& call, bdpt_path_args& a, const unsigned* sid, const int* vlp) {
    // every launch carries its pass table (<= 128 passes: the plan's cap) in the kernel
    // arguments: no upload, no copy kernel (and its gap) before the path kernel
    static_assert(BDPT_DEV_INLINE_PASSES >= 128, "launches of up to 128 passes");
    a.npass = L.npass;
    a.sid = nullptr;
    a.vlp = nullptr;
    for (int q = 0; q < L.npass; q++) {
        a.sid_inl[q] = sid[q];
        a.vlp_inl[q] = vlp[q];
    }
    a.streams = L.streams;
    if (L.unitsl) a.unit_passes = L.unit_passes;
    const hipFunction_t jf = k.jf[L.kernel];
    c->last_specialized = jf != nullptr;
    c->last_features = L.features;
    void* kargs[] = {&a};
    const int half = c->rb_next;
    // the stream of this launch (and of its fold): `stream`, or pstream[half] for an
    // overlapped pooled launch
    hipStream_t ls = c->stream;
    if (L.overlap) {
        ls = c->pstream[half];
        HIPCHK(c, hipStreamWaitEvent(ls, c->amark, 0));
    }
    if (!call.ev0_done) {                                    // the call's time starts here
        HIPCHK(c, hipEventRecord(call.cs->ev0, ls));
        call.ev0_done = true;
    }
    if (L.unitsl) {
        // the units fold in the kernel: no radiance buffer; the previous call's folds were
        // joined in begin_call
        a.rbuf = nullptr;
        a.rmask = nullptr;
    } else if (L.st) {
        // this half was last read by the fold of the launch before the previous one
        if (c->rb_used[half]) HIPCHK(c, hipStreamWaitEvent(ls, c->rb_fold_ev[half], 0));
        a.rbuf = c->d_rbuf + (size_t)half * c->rbuf_cap;
        a.rmask = c->d_rmask + (size_t)half * 4 * c->rmask_lanes;
        // pools mark their stored samples in the mask: cleared first (the fold that read this
        // half ran earlier on this stream)
        if (L.pooled) HIPCHK(c, hipMemsetAsync(a.rmask, 0, 16 * (size_t)plan.lanes, ls));
    } else if (int rc = join_fold(c)) {                      // the fused kernel updates colors itself
        return rc;
    }
    a.pool = 0;
    a.pool_ctr = nullptr;
    if (L.pooled)
        if (int rc = prepare_pool_launch(c, L, ls, half, a)) return rc;
    if (L.unitsl)
        if (int rc = prepare_units_launch(c, plan, L, a)) return rc;
    call.pool_ran |= L.pooled;
    call.units_ran |= L.unitsl;
    const dim3 grid(L.grid[0], L.grid[1], L.grid[2]), block(256);
    HIPCHK(c, hipEventRecord(call.cs->kev[2 * call.launches], ls));
    if (jf)
        HIPCHK(c, hipModuleLaunchKernel(jf, grid.x, grid.y, grid.z, block.x, 1, 1, (unsigned)L.smem, ls, kargs, nullptr));
    else
        HIPCHK(c, hipLaunchKernel(precompiled_path_kernel(plan, L), grid, block, kargs, L.smem, ls));
    HIPCHK(c, hipEventRecord(call.cs->kev[2 * call.launches + 1], ls));
    call.launches++;
    return L.st && !L.unitsl ? issue_fold(c, call, plan.lanes, ls, half, kargs) : BDPT_OK;
}

// Close the call's timing and its ring slot, and tell the tuner what a measuring call ran.
static int end_call(bdpt_ctx* c, const bdpt_plan& plan, const path_kernels& k, const path_call& call, int npass) {
    // the call ends with its last fold (fstream, which waited for the path kernels) if one is
    // outstanding, else on the context's stream
    HIPCHK(c, hipEventRecord(call.cs->ev1, c->fold_pending ? c->fold_stream : c->stream));
    call.cs->launches = call.launches;
    call.cs->pending = true;
    call.cs->serial_fold = call.serial_fold;
    if (plan.tune_role >= 0)
        c->tuner.record(plan.tune_role,
                        bdpt_role_real(plan.tune_role, plan.quarter_ran, k.jf[BDPT_KERNEL_FUSED] != nullptr,
                                       call.pool_ran, call.units_ran),
                        c->issued, npass);
    c->issued++;
    return BDPT_OK;
}

// The tile list of a masked call: the mask's non-zero bytes as tile indices, ascending, kept in the
// call's ring slot until the call has finished and uploaded on the context's stream behind the
// outstanding fold (the previous list's last reader).
static_assert(BDPT_NOISE_TW == BDPT_BTW && BDPT_NOISE_TH == BDPT_BTH, "the mask's tiles are the path kernel's workgroup tiles");
static int upload_tile_list(bdpt_ctx* c, const std::vector<unsigned>& tiles) {
    if (int rc = join_fold(c)) return rc;
    if (tiles.size() > c->tiles_cap) {
        HIPCHK(c, hipStreamSynchronize(c->stream));         // queued launches may read the old buffer
        if (c->d_tiles) HIPCHK(c, hipFree(c->d_tiles));
        c->d_tiles = nullptr;
        c->tiles_cap = 0;
        const size_t cap = (size_t)((c->W + BDPT_BTW - 1) / BDPT_BTW) * ((c->H + BDPT_BTH - 1) / BDPT_BTH);
        if (hipMalloc(&c->d_tiles, sizeof(unsigned) * cap) != hipSuccess)
            return fail(c, BDPT_ENOMEM, "bdpt_path_passes_tiles: tile list (%zu B)", sizeof(unsigned) * cap);
        c->tiles_cap = cap;
    }
    HIPCHK(c, hipMemcpyAsync(c->d_tiles, tiles.data(), sizeof(unsigned) * tiles.size(), hipMemcpyHostToDevice, c->stream));
    return BDPT_OK;
}

static int one_path_passes(bdpt_ctx* c, const unsigned* sid, const int* vlp, int npass, const unsigned char* mask = nullptr) {
    if (!c) return BDPT_EINVAL;
    if (npass < 0 || (npass > 0 && (!sid || !vlp))) return fail(c, BDPT_EINVAL, "bdpt_path_passes: bad pass list");
    if (mask && c->nshards > 1) return fail(c, BDPT_EINVAL, "bdpt_path_passes_tiles: sharded contexts take no tile mask");
    if (npass == 0) return BDPT_OK;
    if (!c->rand_ready) return fail(c, BDPT_ESTATE, "bdpt_path_passes: no random table (run the light pass first)");
    if (!c->cam_set) return fail(c, BDPT_ESTATE, "bdpt_path_passes: camera not set");
    int ntiles = -1;
    if (mask) {
        const size_t nt = (size_t)((c->W + BDPT_BTW - 1) / BDPT_BTW) * ((c->H + BDPT_BTH - 1) / BDPT_BTH);
        ntiles = 0;
        for (size_t t = 0; t < nt; t++) ntiles += mask[t] != 0;
        if (ntiles == 0) return BDPT_OK;                     // nothing to render: no launch, no change
    }
    if (c->cpu) return cpu_path_passes(c, sid, vlp, npass, mask);
    HIPCHK(c, hipSetDevice(c->device));
    // this call's ring slot was last used kRing calls ago: wait for (only) that call
    path_call call;
    call.cs = &c->ring[c->issued % bdpt_ctx::kRing];
    if (int rc = fold_timing(c, c->issued - bdpt_ctx::kRing + 1)) return rc;
    bdpt_path_args a;
    if (int rc = path_args_base(c, a)) return rc;
    if (!mask)                                               // a masked call leaves the tuner as it is
        if (int rc = settle_stream_mode(c)) return rc;

    const bdpt_path_env env = path_env();
    const bdpt_plan_in in = {c->W, c->H, c->shard, c->nshards, c->band_rows, c->streams_req, npass, a.n,
                             c->has_bvh, c->traversal, c->bvh_ns, kBvhAutoSpheres, c->cus, ntiles};
    const bdpt_plan plan = bdpt_plan_call(in, c->tuner, env);
    c->last_streams = plan.S;
    c->last_bvh = plan.bvh;
    path_args_plan(c, plan, a);
    if (mask) {
        std::vector<unsigned>& tiles = call.cs->tiles;
        tiles.clear();
        for (unsigned t = 0; t < (unsigned)(plan.gx * plan.grid_rows); t++)
            if (mask[t]) tiles.push_back(t);
        if (int rc = upload_tile_list(c, tiles)) return rc;
        a.tile_list = c->d_tiles;
        a.ntiles = ntiles;
        a.tiles_per_band = 1;               // no packed edges; one shard: tile row r is grid row r
    }

    while (call.cs->kev.size() < 2 * (size_t)plan.launches) {   // per launch {before, after}
        hipEvent_t e;
        HIPCHK(c, hipEventCreate(&e));
        call.cs->kev.push_back(e);
    }
    path_kernels k;
    if (int rc = resolve_path_kernels(c, plan, npass, a, k)) return rc;
    if (int rc = ensure_radiance_buffers(c, plan, npass, k.jf[BDPT_KERNEL_UNITS] != nullptr)) return rc;
    size_t tab = 0, ids = 0;
    path_lds_table(a, plan.bvh, &tab, &ids);
    if (int rc = check_path_lds(c, plan, k, tab, ids, env, npass, a.n)) return rc;

    if (int rc = begin_call(c, plan, env, k, call)) return rc;
    for (int p0 = 0; call.launches < plan.launches; p0 += plan.chunk) {
        const bdpt_launch L = bdpt_plan_launch(plan, p0, npass, k.jf[BDPT_KERNEL_POOL] != nullptr,
                                               k.jf[BDPT_KERNEL_UNITS] != nullptr, k.jf[BDPT_KERNEL_STREAMS] != nullptr,
                                               k.jf[BDPT_KERNEL_FUSED] != nullptr, k.use_srec, c->jit_zero_exit, tab, ids, env);
        if (int rc = launch_path_kernel(c, plan, L, k, call, a, sid + p0, vlp + p0)) return rc;
    }
    return end_call(c, plan, k, call, npass);
}

// After the stream has drained: did a unit's handover wait time out in a units launch since the
// last check?  Reported once by whichever call looks first (synchronize, the timing calls, the
// read-backs); the error word is then cleared, so later launches report only their own timeouts.
extern "C++" int bdpt_host::units_verdict(bdpt_ctx* c) {
    if (!c->units_check) return BDPT_OK;
    unsigned e = 0;
    HIPCHK(c, hipMemcpy(&e, c->d_uerr, sizeof e, hipMemcpyDeviceToHost));
    c->units_check = false;
    if (!e) return BDPT_OK;
    HIPCHK(c, hipMemset(c->d_uerr, 0, sizeof e));
    return fail(c, BDPT_EHIP, "path kernel: a unit waited too long for its tile's previous range "
                              "(its predecessor did not finish within ~1 s; the frame is not valid)");
}

static int one_synchronize(bdpt_ctx* c) {
    if (!c) return BDPT_EINVAL;
    if (c->cpu) return BDPT_OK;
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = join_fold(c)) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (int rc = units_verdict(c)) return rc;
    return fold_timing(c);
}

int bdpt_last_path_ms(bdpt_ctx* c, float* ms) {
    if (!c || !ms) return BDPT_EINVAL;
    if (int rc = one_synchronize(c)) return rc;
    if (c->acc_launches == 0) return fail(c, BDPT_ESTATE, "bdpt_last_path_ms: no path pass launched");
    *ms = c->last_ms;
    return BDPT_OK;
}

static int one_path_timing(bdpt_ctx* c, double* total_ms, long long* launches, int reset) {
    if (!c) return BDPT_EINVAL;
    if (int rc = one_synchronize(c)) return rc;
    if (total_ms) *total_ms = c->acc_ms;
    if (launches) *launches = c->acc_launches;
    if (reset) { c->acc_ms = 0.0; c->acc_kernel_ms = 0.0; c->acc_launches = 0; }
    return BDPT_OK;
}

static int one_kernel_timing(bdpt_ctx* c, double* kernel_ms, long long* launches, int reset) {
    if (!c) return BDPT_EINVAL;
    if (int rc = one_synchronize(c)) return rc;
    if (kernel_ms) *kernel_ms = c->acc_kernel_ms;
    if (launches) *launches = c->acc_launches;
    if (reset) { c->acc_ms = 0.0; c->acc_kernel_ms = 0.0; c->acc_launches = 0; }
    return BDPT_OK;
}

static int one_read_radiance(bdpt_ctx* c, bdpt_vec* colors, unsigned* counter) {
    if (!c) return BDPT_EINVAL;
    if (c->cpu) {
        bdpt_cpu_read_radiance(c->cpu, colors, counter);
        return BDPT_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = join_fold(c)) return rc;
    const size_t np = (size_t)c->W * c->H;
    if (colors) HIPCHK(c, hipMemcpyAsync(colors, c->d_colors, sizeof(bdpt_vec) * np, hipMemcpyDeviceToHost, c->stream));
    if (counter) HIPCHK(c, hipMemcpyAsync(counter, c->d_counter, sizeof(unsigned) * np, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return units_verdict(c);                                 // a frame known to be invalid is an error
}

static int one_read_pixels(bdpt_ctx* c, unsigned char* rgba) {
    if (!c || !rgba) return BDPT_EINVAL;
    if (c->cpu) {
        bdpt_cpu_read_pixels(c->cpu, rgba);
        return BDPT_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = join_fold(c)) return rc;
    HIPCHK(c, hipMemcpyAsync(rgba, c->d_pixels, 4 * (size_t)c->W * c->H, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return units_verdict(c);
}

int bdpt_read_rand(bdpt_ctx* c, float* t) {
    if (!c || !t) return BDPT_EINVAL;
    if (!c->rand_ready) return fail(c, BDPT_ESTATE, "bdpt_read_rand: table not generated");
    if (c->cpu) {
        bdpt_cpu_read_rand(c->cpu, t);
        return BDPT_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(t, c->d_rand, sizeof(float) * BDPT_RAND_N, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BDPT_OK;
}

// The counterpart of bdpt_read_rand: the table from the host, and what one_generate_rand does after
// the generator (the planar copy; the derived tables are rebuilt on their next use).
int bdpt_write_rand(bdpt_ctx* c, const float* t) {
    if (!c || !t) return BDPT_EINVAL;
    if (c->multi) return fail(c, BDPT_EINVAL, "bdpt_write_rand: multi-device contexts generate their tables");
    if (c->cpu) {
        bdpt_cpu_write_rand(c->cpu, t);
    } else {
        HIPCHK(c, hipSetDevice(c->device));
        if (int rc = join_fold(c)) return rc;              // path kernels read the table
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipMemcpyAsync(c->d_rand, t, sizeof(float) * BDPT_RAND_N, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(bdpt_rand_planar_kernel, dim3((BDPT_DEV_RANDP_PLANES * BDPT_DEV_RANDP_PL + 255) / 256),
                           dim3(256), 0, c->stream, (const float*)c->d_rand, c->d_rndp);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->scp_ready = c->srec_ready = false;
    }
    c->rand_ready = true;
    c->rand_uploaded = true;
    return BDPT_OK;
}

int bdpt_read_sample_records(bdpt_ctx* c, float* rec) {
    if (!c || !rec) return BDPT_EINVAL;
    if (c->cpu) return fail(c, BDPT_EINVAL, "bdpt_read_sample_records: the CPU backend has no sample records");
    if (!c->rand_ready) return fail(c, BDPT_ESTATE, "bdpt_read_sample_records: table not generated");
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = ensure_srec(c)) return rc;
    const size_t half = BDPT_DEV_SREC_HALF;
    std::vector<float4> h(2 * half);
    HIPCHK(c, hipMemcpyAsync(h.data(), c->d_srec, sizeof(float4) * h.size(), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (size_t j = 0; j < (size_t)BDPT_RAND_N - 5; j++) {     // table order: 8 floats per position
        const size_t e = (j % 25) * BDPT_DEV_RANDP_PL + j / 25;
        memcpy(rec + 8 * j, &h[e], sizeof(float4));
        memcpy(rec + 8 * j + 4, &h[half + e], sizeof(float4));
    }
    return BDPT_OK;
}

int bdpt_read_lightpaths(bdpt_ctx* c, bdpt_lightpath* lp) {
    if (!c || !lp) return BDPT_EINVAL;
    if (c->cpu) {
        bdpt_cpu_read_lightpaths(c->cpu, lp);
        return BDPT_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(lp, c->d_lp, sizeof(bdpt_lightpath) * BDPT_LIGHT_POINTS, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BDPT_OK;
}

static int one_write_lightpaths(bdpt_ctx* c, const bdpt_lightpath* lp) {
    if (!c || !lp) return BDPT_EINVAL;
    if (c->cpu) {
        bdpt_cpu_write_lightpaths(c->cpu, lp);
        return BDPT_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    // queued passes may still read dev_lp: overlapped pooled launches run on the pstreams, which
    // `stream` follows only through the last fold
    if (int rc = join_fold(c)) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_lp, lp, sizeof(bdpt_lightpath) * BDPT_LIGHT_POINTS, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BDPT_OK;
}

int bdpt_rand_seed(const bdpt_ctx* c, unsigned* seed) {
    if (!c || !seed) return BDPT_EINVAL;
    if (!c->rand_ready || c->rand_uploaded) return BDPT_ESTATE;
    *seed = c->rand_seed;
    return BDPT_OK;
}

int bdpt_get_camera(const bdpt_ctx* c, bdpt_camera* cam) {
    if (!c || !cam) return BDPT_EINVAL;
    if (!c->cam_set) return BDPT_ESTATE;
    *cam = c->cam;
    return BDPT_OK;
}

int bdpt_get_scene(const bdpt_ctx* c, bdpt_sphere* spheres, unsigned cap) {
    if (!c) return BDPT_EINVAL;
    const unsigned n = (unsigned)c->spheres.size();
    if (spheres)
        for (unsigned i = 0; i < n && i < cap; i++) spheres[i] = c->spheres[i];
    return (int)n;
}

int bdpt_frame_size(const bdpt_ctx* c, int* W, int* H) {
    if (!c || !W || !H) return BDPT_EINVAL;
    *W = c->W;
    *H = c->H;
    return BDPT_OK;
}

int bdpt_last_kernel_features(const bdpt_ctx* c) { return c ? c->last_features : BDPT_EINVAL; }

int bdpt_path_lds(const bdpt_ctx* c, unsigned* static_bytes, unsigned* dynamic_bytes, unsigned* limit_bytes) {
    if (!c) return BDPT_EINVAL;
    if (static_bytes) *static_bytes = (unsigned)c->last_lds_static;
    if (dynamic_bytes) *dynamic_bytes = (unsigned)c->last_lds_dynamic;
    if (limit_bytes) *limit_bytes = (unsigned)c->lds_limit;
    return BDPT_OK;
}

static int one_device_buffers(bdpt_ctx* c, void** colors, void** counter, void** pixels) {
    if (!c) return BDPT_EINVAL;
    if (c->cpu) return fail(c, BDPT_EINVAL, "bdpt_device_buffers: the CPU backend has no device buffers");
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = join_fold(c)) return rc;                   // work queued on the stream follows the fold
    if (colors) *colors = c->d_colors;
    if (counter) *counter = c->d_counter;
    if (pixels) *pixels = c->d_pixels;
    return BDPT_OK;
}

static int one_update_pixels(bdpt_ctx* c) {
    if (!c) return BDPT_EINVAL;
    if (c->cpu) {
        bdpt_cpu_update_pixels(c->cpu);
        return BDPT_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = join_fold(c)) return rc;
    const int np = c->W * c->H;
    hipLaunchKernelGGL(bdpt_pixels_kernel, dim3((np + 255) / 256), dim3(256), 0, c->stream,
                       (const bdpt_dev_vec*)c->d_colors, c->d_pixels, (const float*)c->d_thr, np);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BDPT_OK;
}

}  // extern "C"

// ---- multi-device contexts (SURVEY.md 8(b) `devices[], ndev`; 5: RCCL in one process) --------
// bdpt_create_multi makes one context per device: the first renders on devices[0] and owns the
// others (peers).  Device k renders the 8-row bands (y / 8) % ndev == k; every other entry point
// applies to all devices (each rebuilds the MT table and the VLPs itself: they are deterministic),
// and the read-back entry points first assemble the frame on devices[0]: an in-process RCCL
// ncclReduce (sum) of the float radiance and the counters over ncclCommInitAll's communicator
// (the sum is exact, each pixel is non-zero on one device only), or, when the devices are not
// distinct (several shards on one GPU) or RCCL is unavailable, peer copies plus an add kernel.
namespace {
struct rccl_api {
    bool ok = false;
    decltype(&ncclCommInitAll) init_all = nullptr;
    decltype(&ncclCommDestroy) destroy = nullptr;
    decltype(&ncclReduce) reduce = nullptr;
    decltype(&ncclGroupStart) group_start = nullptr;
    decltype(&ncclGroupEnd) group_end = nullptr;
    decltype(&ncclGetErrorString) errstr = nullptr;
    decltype(&ncclGetVersion) version = nullptr;       // optional (reporting only)
};

const rccl_api& rccl() {
    static const rccl_api api = [] {
        rccl_api r;
        // torch (when loaded) has mapped its own librccl.so.1 already: the same SONAME binds to it
        const char* libs[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
        void* h = nullptr;
        for (const char* l : libs)
            if ((h = dlopen(l, RTLD_NOW | RTLD_LOCAL))) break;
        if (!h) return r;
        r.init_all = (decltype(r.init_all))dlsym(h, "ncclCommInitAll");
        r.destroy = (decltype(r.destroy))dlsym(h, "ncclCommDestroy");
        r.reduce = (decltype(r.reduce))dlsym(h, "ncclReduce");
        r.group_start = (decltype(r.group_start))dlsym(h, "ncclGroupStart");
        r.group_end = (decltype(r.group_end))dlsym(h, "ncclGroupEnd");
        r.errstr = (decltype(r.errstr))dlsym(h, "ncclGetErrorString");
        r.version = (decltype(r.version))dlsym(h, "ncclGetVersion");
        r.ok = r.init_all && r.destroy && r.reduce && r.group_start && r.group_end && r.errstr;
        return r;
    }();
    return api;
}

// The group bracket of the in-process frame reduce: every device's two ncclReduce calls between
// one ncclGroupStart and one ncclGroupEnd.  A failed hipSetDevice or ncclReduce stops issuing but
// still closes the group (an open group would make the next RCCL call on the communicators fail
// with an unrelated error); the first error is returned in *he / the result.  Templated on the
// calls so that tests can drive it with injected failures (bdpt__test_reduce_bracket).
template <class Start, class End, class SetDev, class Reduce>
ncclResult_t reduce_bracket(int ndev, Start start, End end, SetDev set_device, Reduce reduce, hipError_t* he) {
    *he = hipSuccess;
    ncclResult_t r = start();
    if (r != ncclSuccess) return r;                   // no group was opened
    for (int k = 0; k < ndev && r == ncclSuccess && *he == hipSuccess; k++) {
        *he = set_device(k);
        if (*he != hipSuccess) break;
        r = reduce(k, 0);                             // colours
        if (r == ncclSuccess) r = reduce(k, 1);       // counters
    }
    const ncclResult_t e = end();                     // always: the group is closed
    return r != ncclSuccess ? r : e;
}
}  // namespace

static void destroy_group(bdpt_ctx* c) {
    if (!c->multi) return;
    for (bdpt_ctx* p : c->peers) {
        (void)hipSetDevice(p->device);
        if (p->fstream) (void)hipStreamSynchronize(p->fstream);
        if (p->stream) (void)hipStreamSynchronize(p->stream);
    }
    if (!c->comms.empty() && rccl().ok)
        for (void* cm : c->comms) (void)rccl().destroy((ncclComm_t)cm);
    c->comms.clear();
    for (bdpt_ctx* p : c->peers) bdpt_destroy(p);
    c->peers.clear();
}

// Apply `f` to every peer; the first failure is reported on the group context.
template <class F>
static int forward(bdpt_ctx* c, F f) {
    for (bdpt_ctx* p : c->peers)
        if (int rc = f(p)) return fail(c, rc, "device %d: %s", p->device, p->err);
    c->frame_stale = true;
    return BDPT_OK;
}

// Group shard layout: device k of a group that is shard `shard` of `nshards` groups renders
// shard shard * ndev + k of nshards * ndev.
static int group_set_shard(bdpt_ctx* c, int shard, int nshards, int band_rows) {
    const int ndev = 1 + (int)c->peers.size();
    if (int rc = one_set_shard(c, shard * ndev, nshards * ndev, band_rows)) return rc;
    for (int k = 1; k < ndev; k++)
        if (int rc = one_set_shard(c->peers[k - 1], shard * ndev + k, nshards * ndev, band_rows))
            return fail(c, rc, "device %d: %s", c->peers[k - 1]->device, c->peers[k - 1]->err);
    c->frame_stale = true;
    return BDPT_OK;
}

// Assemble the frame of a multi-device context on devices[0] (d_fcolors/d_fcounter/d_fpixels).
static int assemble(bdpt_ctx* c) {
    if (!c->multi || !c->frame_stale) return BDPT_OK;
    if (int rc = one_synchronize(c)) return rc;
    for (bdpt_ctx* p : c->peers)
        if (int rc = one_synchronize(p)) return fail(c, rc, "device %d: %s", p->device, p->err);
    const size_t np = (size_t)c->W * c->H;
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->d_fcolors) {
        HIPCHK(c, hipMalloc(&c->d_fcolors, sizeof(bdpt_dev_vec) * np));
        HIPCHK(c, hipMalloc(&c->d_fcounter, sizeof(unsigned) * np));
        HIPCHK(c, hipMalloc(&c->d_fpixels, sizeof(uchar4) * np));
    }
    if (c->reduce_mode == kReduceRccl) {
        const rccl_api& api = rccl();
        auto dev = [&](int k) { return k == 0 ? c : c->peers[k - 1]; };
        hipError_t he = hipSuccess;
        const ncclResult_t r = reduce_bracket(
            (int)c->comms.size(), [&] { return api.group_start(); }, [&] { return api.group_end(); },
            [&](int k) { return hipSetDevice(dev(k)->device); },
            [&](int k, int what) {
                bdpt_ctx* d = dev(k);
                return what == 0
                    ? api.reduce(d->d_colors, k == 0 ? (void*)c->d_fcolors : (void*)d->d_colors, 3 * np, ncclFloat32,
                                 ncclSum, 0, (ncclComm_t)c->comms[k], d->stream)
                    : api.reduce(d->d_counter, k == 0 ? (void*)c->d_fcounter : (void*)d->d_counter, np, ncclUint32,
                                 ncclSum, 0, (ncclComm_t)c->comms[k], d->stream);
            },
            &he);
        (void)hipSetDevice(c->device);
        if (he != hipSuccess) return fail(c, BDPT_EHIP, "frame reduce: hipSetDevice: %s", hipGetErrorString(he));
        if (r != ncclSuccess) return fail(c, BDPT_EHIP, "ncclReduce: %s", api.errstr(r));
        for (size_t k = 1; k < c->comms.size(); k++) {
            HIPCHK(c, hipSetDevice(c->peers[k - 1]->device));
            HIPCHK(c, hipStreamSynchronize(c->peers[k - 1]->stream));
        }
        HIPCHK(c, hipSetDevice(c->device));
    } else {
        HIPCHK(c, hipMemcpyAsync(c->d_fcolors, c->d_colors, sizeof(bdpt_dev_vec) * np, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->d_fcounter, c->d_counter, sizeof(unsigned) * np, hipMemcpyDeviceToDevice, c->stream));
        if (!c->peers.empty() && !c->d_ftmp) {
            HIPCHK(c, hipMalloc(&c->d_ftmp, sizeof(bdpt_dev_vec) * np));
            HIPCHK(c, hipMalloc(&c->d_ftmpc, sizeof(unsigned) * np));
        }
        for (bdpt_ctx* p : c->peers) {
            HIPCHK(c, hipMemcpyPeerAsync(c->d_ftmp, c->device, p->d_colors, p->device, sizeof(bdpt_dev_vec) * np, c->stream));
            HIPCHK(c, hipMemcpyPeerAsync(c->d_ftmpc, c->device, p->d_counter, p->device, sizeof(unsigned) * np, c->stream));
            hipLaunchKernelGGL(bdpt_frame_add_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, c->stream,
                               (float*)c->d_fcolors, (const float*)c->d_ftmp, c->d_fcounter,
                               (const unsigned*)c->d_ftmpc, (int)np);
            HIPCHK(c, hipGetLastError());
        }
    }
    hipLaunchKernelGGL(bdpt_pixels_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, c->stream,
                       (const bdpt_dev_vec*)c->d_fcolors, c->d_fpixels, (const float*)c->d_thr, (int)np);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->frame_stale = false;
    return BDPT_OK;
}

extern "C" {

int bdpt_create_multi(bdpt_ctx** out, const bdpt_sphere* spheres, unsigned n, int W, int H,
                      const char* mt_dat_path, const int* devices, int ndev) {
    if (!out) return BDPT_EINVAL;
    *out = nullptr;
    bool has_cpu = false;
    for (int k = 0; devices && k < ndev && k < 64; k++) has_cpu = has_cpu || devices[k] < 0;
    if (!devices || ndev < 1 || ndev > 64 || has_cpu) {
        snprintf(g_create_err, sizeof g_create_err, "bdpt_create_multi: bad device list (%d devices)", ndev);
        return BDPT_EINVAL;
    }
    bdpt_ctx* c = nullptr;
    if (int rc = bdpt_create(&c, spheres, n, W, H, mt_dat_path, devices[0])) return rc;
    c->multi = true;
    for (int k = 1; k < ndev; k++) {
        bdpt_ctx* p = nullptr;
        if (int rc = bdpt_create(&p, spheres, n, W, H, mt_dat_path, devices[k])) {
            char msg[512];
            snprintf(msg, sizeof msg, "device %d: %s", devices[k], g_create_err);
            bdpt_destroy(c);
            snprintf(g_create_err, sizeof g_create_err, "%s", msg);
            return rc;
        }
        p->group_leader = c;
        c->peers.push_back(p);
    }
    if (int rc = group_set_shard(c, 0, 1, 8)) {
        snprintf(g_create_err, sizeof g_create_err, "%s", c->err);
        bdpt_destroy(c);
        return rc;
    }
    // RCCL when every device is distinct (a communicator holds each GPU once), else peer copies
    bool distinct = true;
    for (int a = 0; a < ndev; a++)
        for (int b = a + 1; b < ndev; b++) distinct = distinct && devices[a] != devices[b];
    const char* force = getenv("BDPT_REDUCE");
    c->reduce_mode = kReducePeer;
    if (force && !strcmp(force, "peer")) {
        snprintf(c->reduce_note, sizeof c->reduce_note, "BDPT_REDUCE=peer");
    } else if (!distinct) {
        snprintf(c->reduce_note, sizeof c->reduce_note, "devices repeat: peer copies");
    } else if (!rccl().ok) {
        snprintf(c->reduce_note, sizeof c->reduce_note, "librccl not found: peer copies");
    } else {
        std::vector<ncclComm_t> comms(ndev);
        const ncclResult_t r = rccl().init_all(comms.data(), ndev, devices);
        if (r == ncclSuccess) {
            c->comms.assign(comms.begin(), comms.end());
            c->reduce_mode = kReduceRccl;
            const int v = bdpt_rccl_version();
            std::string ids;
            for (int k = 0; k < ndev; k++) ids += (k ? " " : "") + std::to_string(devices[k]);
            snprintf(c->reduce_note, sizeof c->reduce_note, "rccl %d.%d.%d, ncclCommInitAll: %d ranks on devices [%s]",
                     v / 10000, v / 100 % 100, v % 100, ndev, ids.c_str());
        } else {
            snprintf(c->reduce_note, sizeof c->reduce_note, "ncclCommInitAll: %s: peer copies", rccl().errstr(r));
        }
    }
    (void)hipSetDevice(devices[0]);
    *out = c;
    return BDPT_OK;
}

int bdpt_num_devices(const bdpt_ctx* c) { return c ? 1 + (int)c->peers.size() : BDPT_EINVAL; }

int bdpt_rccl_version(void) {
    const rccl_api& api = rccl();
    if (!api.ok) return BDPT_ESTATE;
    int v = 0;
    if (!api.version || api.version(&v) != ncclSuccess) return BDPT_ESTATE;
    return v;
}

int bdpt_reduce_info(const bdpt_ctx* c, char* buf, int cap) {
    if (!c || !buf || cap < 1) return BDPT_EINVAL;
    const char* s = !c->multi ? "none: one device" : c->reduce_note;
    snprintf(buf, (size_t)cap, "%s", s);
    return (int)strlen(s);
}

// Test hook (tests/test_abi_host.py): the reduce bracket driven by fake calls on `ndev` devices,
// hipSetDevice failing on device `fail_dev` and ncclReduce on call `fail_reduce` (-1: never).
// Returns the bracket's ncclResult_t; *open_groups = group starts minus ends afterwards (0: the
// group was closed), *reduces = ncclReduce calls issued, *hip_err = the hipError_t it reported.
int bdpt__test_reduce_bracket(int ndev, int fail_dev, int fail_reduce, int* open_groups, int* reduces,
                              int* hip_err) {
    int open = 0, calls = 0;
    hipError_t he = hipSuccess;
    const ncclResult_t r = reduce_bracket(
        ndev, [&] { open++; return ncclSuccess; }, [&] { open--; return ncclSuccess; },
        [&](int k) { return k == fail_dev ? hipErrorInvalidDevice : hipSuccess; },
        [&](int, int) { return calls++ == fail_reduce ? ncclUnhandledCudaError : ncclSuccess; }, &he);
    if (open_groups) *open_groups = open;
    if (reduces) *reduces = calls;
    if (hip_err) *hip_err = (int)he;
    return (int)r;
}

const char* bdpt_reduce_backend(const bdpt_ctx* c) {
    if (!c) return "null context";
    if (!c->multi) return "none";
    return c->reduce_mode == kReduceRccl ? "rccl" : "peer";
}

int bdpt_reduce_frame(bdpt_ctx* c) {
    if (!c) return BDPT_EINVAL;
    return assemble(c);
}

// ---- the entry points: this context, then (multi-device) every peer ------------------------
int bdpt_set_scene(bdpt_ctx* c, const bdpt_sphere* spheres, unsigned n) {
    if (int rc = one_set_scene(c, spheres, n)) return rc;
    return forward(c, [&](bdpt_ctx* p) { return one_set_scene(p, spheres, n); });
}
int bdpt_set_camera(bdpt_ctx* c, const bdpt_camera* cam) {
    if (int rc = one_set_camera(c, cam)) return rc;
    return forward(c, [&](bdpt_ctx* p) { return one_set_camera(p, cam); });
}
int bdpt_reset_accum(bdpt_ctx* c) {
    if (int rc = one_reset_accum(c)) return rc;
    return forward(c, [&](bdpt_ctx* p) { return one_reset_accum(p); });
}
int bdpt_set_shard(bdpt_ctx* c, int shard, int nshards, int band_rows) {
    if (!c) return BDPT_EINVAL;
    if (!c->multi) return one_set_shard(c, shard, nshards, band_rows);
    if (nshards < 1 || shard < 0 || shard >= nshards || band_rows < 1)
        return fail(c, BDPT_EINVAL, "bdpt_set_shard: bad shard %d/%d band %d", shard, nshards, band_rows);
    return group_set_shard(c, shard, nshards, band_rows);
}
int bdpt_set_streams(bdpt_ctx* c, int streams) {
    if (int rc = one_set_streams(c, streams)) return rc;
    return forward(c, [&](bdpt_ctx* p) { return one_set_streams(p, streams); });
}
int bdpt_set_stream_choice(bdpt_ctx* c, int choice) {
    if (int rc = one_set_stream_choice(c, choice)) return rc;
    return forward(c, [&](bdpt_ctx* p) { return one_set_stream_choice(p, choice); });
}
// One device of the group: the kernel its last path-pass call ran and its stream-mode choice.
int bdpt_device_mode(bdpt_ctx* c, int k, int* last_streams, int* features, int* choice) {
    if (!c) return BDPT_EINVAL;
    if (k < 0 || k > (int)c->peers.size())
        return fail(c, BDPT_EINVAL, "bdpt_device_mode: device index %d of %d", k, 1 + (int)c->peers.size());
    const bdpt_ctx* d = k == 0 ? c : c->peers[k - 1];
    if (last_streams) *last_streams = d->last_streams;
    if (features) *features = d->last_features;
    if (choice) *choice = choice_of(d);
    return BDPT_OK;
}
int bdpt_set_specialize(bdpt_ctx* c, int on) {
    if (int rc = one_set_specialize(c, on)) return rc;
    return forward(c, [&](bdpt_ctx* p) { return one_set_specialize(p, on); });
}
int bdpt_set_traversal(bdpt_ctx* c, int mode) {
    if (int rc = one_set_traversal(c, mode)) return rc;
    return forward(c, [&](bdpt_ctx* p) { return one_set_traversal(p, mode); });
}
int bdpt_generate_rand(bdpt_ctx* c, unsigned seed) {
    if (int rc = one_generate_rand(c, seed)) return rc;
    return forward(c, [&](bdpt_ctx* p) { return one_generate_rand(p, seed); });
}
int bdpt_light_pass(bdpt_ctx* c, int current_sample) {
    if (int rc = one_light_pass(c, current_sample)) return rc;
    return forward(c, [&](bdpt_ctx* p) { return one_light_pass(p, current_sample); });
}
// Every device's passes are queued before any is waited for: the devices render concurrently.
int bdpt_path_passes(bdpt_ctx* c, const unsigned* sid, const int* vlp, int npass) {
    if (int rc = one_path_passes(c, sid, vlp, npass)) return rc;
    return forward(c, [&](bdpt_ctx* p) { return one_path_passes(p, sid, vlp, npass); });
}
int bdpt_path_passes_tiles(bdpt_ctx* c, const unsigned* sid, const int* vlp, int npass, const unsigned char* tile_mask) {
    if (!tile_mask) return bdpt_path_passes(c, sid, vlp, npass);
    if (!c) return BDPT_EINVAL;
    if (c->multi) return fail(c, BDPT_EINVAL, "bdpt_path_passes_tiles: multi-device contexts take no tile mask");
    return one_path_passes(c, sid, vlp, npass, tile_mask);
}
int bdpt_synchronize(bdpt_ctx* c) {
    if (int rc = one_synchronize(c)) return rc;
    for (bdpt_ctx* p : c->peers)
        if (int rc = one_synchronize(p)) return fail(c, rc, "device %d: %s", p->device, p->err);
    return BDPT_OK;
}
// How many path-pass calls the GPU has not finished: the ring slots not folded yet whose closing
// event has not fired.  Only queries: no wait, no timing folded, nothing issued.
static int one_calls_in_flight(bdpt_ctx* c, int* n) {
    if (c->cpu) return BDPT_OK;
    HIPCHK(c, hipSetDevice(c->device));
    for (const bdpt_ctx::call_slot& s : c->ring) {
        if (!s.pending) continue;
        const hipError_t e = hipEventQuery(s.ev1);
        if (e == hipErrorNotReady) {
            (void)hipGetLastError();                         // not-ready is an answer, not an error to keep
            ++*n;
        } else if (e != hipSuccess) {
            return fail(c, BDPT_EHIP, "hipEventQuery: %s", hipGetErrorString(e));
        }
    }
    return BDPT_OK;
}
int bdpt_calls_in_flight(bdpt_ctx* c, int* n) {
    if (!c || !n) return BDPT_EINVAL;
    *n = 0;
    if (int rc = one_calls_in_flight(c, n)) return rc;
    for (bdpt_ctx* p : c->peers)
        if (int rc = one_calls_in_flight(p, n)) return fail(c, rc, "device %d: %s", p->device, p->err);
    return BDPT_OK;
}
// Multi-device: the slowest device's time (the devices run concurrently); launches of devices[0].
int bdpt_path_timing(bdpt_ctx* c, double* total_ms, long long* launches, int reset) {
    if (int rc = one_path_timing(c, total_ms, launches, reset)) return rc;
    for (bdpt_ctx* p : c->peers) {
        double ms = 0.0;
        if (int rc = one_path_timing(p, &ms, nullptr, reset)) return fail(c, rc, "device %d: %s", p->device, p->err);
        if (total_ms && ms > *total_ms) *total_ms = ms;
    }
    return BDPT_OK;
}
int bdpt_kernel_timing(bdpt_ctx* c, double* kernel_ms, long long* launches, int reset) {
    if (int rc = one_kernel_timing(c, kernel_ms, launches, reset)) return rc;
    for (bdpt_ctx* p : c->peers) {
        double ms = 0.0;
        if (int rc = one_kernel_timing(p, &ms, nullptr, reset)) return fail(c, rc, "device %d: %s", p->device, p->err);
        if (kernel_ms && ms > *kernel_ms) *kernel_ms = ms;
    }
    return BDPT_OK;
}
// One device of the group (k = 0 is devices[0]): its own accumulators, not the maximum, so a
// multi-device run can show load imbalance.  Does not reset.
int bdpt_device_timing(bdpt_ctx* c, int k, int* device, double* kernel_ms, double* path_ms,
                       long long* launches, long long* owned_pixels) {
    if (!c) return BDPT_EINVAL;
    if (k < 0 || k > (int)c->peers.size())
        return fail(c, BDPT_EINVAL, "bdpt_device_timing: device index %d of %d", k, 1 + (int)c->peers.size());
    bdpt_ctx* d = k == 0 ? c : c->peers[k - 1];
    if (int rc = one_synchronize(d)) return d == c ? rc : fail(c, rc, "device %d: %s", d->device, d->err);
    if (device) *device = d->cpu ? BDPT_DEVICE_CPU : d->device;
    if (kernel_ms) *kernel_ms = d->acc_kernel_ms;
    if (path_ms) *path_ms = d->acc_ms;
    if (launches) *launches = d->acc_launches;
    if (owned_pixels) {
        long long rows = 0;
        for (int y = 0; y < d->H; y++) rows += (y / d->band_rows) % d->nshards == d->shard;
        *owned_pixels = rows * d->W;
    }
    return BDPT_OK;
}
// Read-back of a multi-device context reads the assembled frame.
int bdpt_write_lightpaths(bdpt_ctx* c, const bdpt_lightpath* lp) {
    if (int rc = one_write_lightpaths(c, lp)) return rc;
    return forward(c, [&](bdpt_ctx* p) { return one_write_lightpaths(p, lp); });
}
int bdpt_read_radiance(bdpt_ctx* c, bdpt_vec* colors, unsigned* counter) {
    if (!c) return BDPT_EINVAL;
    if (!c->multi) return one_read_radiance(c, colors, counter);
    if (int rc = assemble(c)) return rc;
    const size_t np = (size_t)c->W * c->H;
    if (colors) HIPCHK(c, hipMemcpyAsync(colors, c->d_fcolors, sizeof(bdpt_vec) * np, hipMemcpyDeviceToHost, c->stream));
    if (counter) HIPCHK(c, hipMemcpyAsync(counter, c->d_fcounter, sizeof(unsigned) * np, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BDPT_OK;
}
int bdpt_read_pixels(bdpt_ctx* c, unsigned char* rgba) {
    if (!c || !rgba) return BDPT_EINVAL;
    if (!c->multi) return one_read_pixels(c, rgba);
    if (int rc = assemble(c)) return rc;
    HIPCHK(c, hipMemcpyAsync(rgba, c->d_fpixels, 4 * (size_t)c->W * c->H, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BDPT_OK;
}
int bdpt_device_buffers(bdpt_ctx* c, void** colors, void** counter, void** pixels) {
    if (!c) return BDPT_EINVAL;
    if (!c->multi) return one_device_buffers(c, colors, counter, pixels);
    if (int rc = assemble(c)) return rc;
    if (colors) *colors = c->d_fcolors;
    if (counter) *counter = c->d_fcounter;
    if (pixels) *pixels = c->d_fpixels;
    return BDPT_OK;
}
int bdpt_update_pixels(bdpt_ctx* c) {
    if (!c) return BDPT_EINVAL;
    if (!c->multi) return one_update_pixels(c);
    return assemble(c);
}

// ---- checkpoint / resume of the accumulation ----------------------------------
// Upload colors/counter (the counterpart of bdpt_read_radiance) and recompute the pixels.  A
// multi-device context gives each device only the pixels of its own bands (zeros elsewhere), so
// the assembled frame is the uploaded one.
static int one_write_radiance(bdpt_ctx* c, const bdpt_vec* colors, const unsigned* counter, bool masked) {
    c->mark_live = false;
    if (c->cpu) {
        bdpt_cpu_write_radiance(c->cpu, colors, counter);
        return BDPT_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = join_fold(c)) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const size_t np = (size_t)c->W * c->H;
    std::vector<bdpt_vec> col;
    std::vector<unsigned> cnt;
    if (masked) {
        col.assign(colors, colors + np);
        cnt.assign(counter, counter + np);
        for (int y = 0; y < c->H; y++) {
            if ((y / c->band_rows) % c->nshards == c->shard) continue;
            memset(&col[(size_t)y * c->W], 0, sizeof(bdpt_vec) * c->W);
            memset(&cnt[(size_t)y * c->W], 0, sizeof(unsigned) * c->W);
        }
        colors = col.data();
        counter = cnt.data();
    }
    HIPCHK(c, hipMemcpyAsync(c->d_colors, colors, sizeof(bdpt_vec) * np, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_counter, counter, sizeof(unsigned) * np, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(bdpt_pixels_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, c->stream,
                       (const bdpt_dev_vec*)c->d_colors, c->d_pixels, (const float*)c->d_thr, (int)np);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BDPT_OK;
}

int bdpt_write_radiance(bdpt_ctx* c, const bdpt_vec* colors, const unsigned* counter) {
    if (!c || !colors || !counter) return BDPT_EINVAL;
    if (int rc = one_write_radiance(c, colors, counter, c->multi)) return rc;
    return forward(c, [&](bdpt_ctx* p) { return one_write_radiance(p, colors, counter, true); });
}

// ---- optional display: HIP-GL interop of the window's pixel-unpack buffer ----
// The reference registers its PBO once (cudaGLRegisterBufferObject, smallpt_cpu.c:112-123) and per
// frame maps it, lets the path kernel write pixels_buf = the mapped pointer, and unmaps it
// (IdleFunc, display_func.c:199-215).  Here the kernels keep writing d_pixels (the read-back,
// checkpoint and multi-device paths all read it) and a publish copies the finished frame into the
// mapped buffer on the context's stream: one 4*W*H-byte device copy per displayed frame (8.3 MB
// at 1080p, ~2 us of HBM time), the same bytes in the same bottom-row-first order.
//
// hipGraphicsGLRegisterBuffer needs an OpenGL context current on the calling thread; without one
// it is undefined what the runtime does, so the context is looked up first (GLX, then EGL) in
// libraries the process has already loaded -- libbdpt itself never links or loads OpenGL.
static bool gl_context_current() {
    typedef void* (*cur_fn)(void);
    const char* const libs[2] = {"libGL.so.1", "libEGL.so.1"};
    const char* const syms[2] = {"glXGetCurrentContext", "eglGetCurrentContext"};
    for (int k = 0; k < 2; k++) {
        cur_fn f = (cur_fn)dlsym(RTLD_DEFAULT, syms[k]);
        void* h = nullptr;
        if (!f && (h = dlopen(libs[k], RTLD_LAZY | RTLD_NOLOAD)) != nullptr) f = (cur_fn)dlsym(h, syms[k]);
        const bool cur = f && f() != nullptr;
        if (h) dlclose(h);
        if (cur) return true;
    }
    return false;
}

int bdpt_gl_register_pbo(bdpt_ctx* c, unsigned pbo) {
    if (!c) return BDPT_EINVAL;
    if (c->cpu) return fail(c, BDPT_EINVAL, "bdpt_gl_register_pbo: the CPU backend has no device pixels");
    if (!pbo) return fail(c, BDPT_EINVAL, "bdpt_gl_register_pbo: buffer name 0");
    if (!gl_context_current())
        return fail(c, BDPT_EINVAL, "bdpt_gl_register_pbo: no OpenGL context is current on this thread");
    HIPCHK(c, hipSetDevice(c->device));
    if (c->gl_res) {
        HIPCHK(c, hipGraphicsUnregisterResource(c->gl_res));
        c->gl_res = nullptr;
        c->gl_pbo = 0;
    }
    hipGraphicsResource_t res = nullptr;                        // kept only on success
    HIPCHK(c, hipGraphicsGLRegisterBuffer(&res, pbo, hipGraphicsRegisterFlagsWriteDiscard));
    c->gl_res = res;
    c->gl_pbo = pbo;
    return BDPT_OK;
}

int bdpt_gl_publish(bdpt_ctx* c) {
    if (!c) return BDPT_EINVAL;
    if (!c->gl_res) return fail(c, BDPT_ESTATE, "bdpt_gl_publish: no buffer registered (bdpt_gl_register_pbo)");
    void* pix = nullptr;
    if (int rc = bdpt_device_buffers(c, nullptr, nullptr, &pix)) return rc;   // multi: the assembled frame
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipGraphicsMapResources(1, &c->gl_res, c->stream));
    // from here the buffer is mapped: every path below unmaps it before returning
    const size_t bytes = 4 * (size_t)c->W * c->H;
    void* dst = nullptr;
    size_t size = 0;
    hipError_t e = hipGraphicsResourceGetMappedPointer(&dst, &size, c->gl_res);
    bool small = false;
    if (e == hipSuccess && size < bytes) small = true;
    else if (e == hipSuccess) e = hipMemcpyAsync(dst, pix, bytes, hipMemcpyDeviceToDevice, c->stream);
    const hipError_t u = hipGraphicsUnmapResources(1, &c->gl_res, c->stream);
    if (small)
        return fail(c, BDPT_EINVAL, "bdpt_gl_publish: buffer %u holds %zu bytes, the frame needs %zu",
                    c->gl_pbo, size, bytes);
    if (e != hipSuccess) return fail(c, BDPT_EHIP, "bdpt_gl_publish: mapped copy: %s", hipGetErrorString(e));
    if (u != hipSuccess) return fail(c, BDPT_EHIP, "bdpt_gl_publish: unmap: %s", hipGetErrorString(u));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return BDPT_OK;
}

int bdpt_gl_unregister(bdpt_ctx* c) {
    if (!c) return BDPT_EINVAL;
    if (!c->gl_res) return BDPT_OK;
    HIPCHK(c, hipSetDevice(c->device));
    hipGraphicsResource_t r = c->gl_res;
    c->gl_res = nullptr;
    c->gl_pbo = 0;
    HIPCHK(c, hipGraphicsUnregisterResource(r));
    return BDPT_OK;
}

// bdpt_save_checkpoint / bdpt_load_checkpoint: bdpt_ckpt.c (over the entry points above)
int bdpt__fail(bdpt_ctx* c, int code, const char* msg) { return fail(c, code, "%s", msg); }

}  // extern "C"


