// bdpt_ctx.h -- private to the host layer: the context behind include/bdpt.h's opaque bdpt_ctx, the
// error helpers, and the few functions that bdpt_host.cpp, bdpt_jit.cpp and the frame services of
// bdpt_frame.cpp call across files.  Nothing here is ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_gl_interop.h>         // hipGraphicsResource_t (the optional display, 8(f)4)
#include <stdarg.h>
#include <stdio.h>
#include <map>
#include <string>
#include <vector>

#include "../../include/bdpt.h"
#include "bdpt_device.h"
#include "bdpt_cpu.h"
#include "bdpt_plan.h"
#include "bdpt_jit_plan.h"

// "The last call's time" of one frame service (bdpt_frame.cpp svc_*; read by bdpt_last_*_ms).
struct bdpt_svc_clock {
    hipEvent_t ev[2] = {nullptr, nullptr};   // around the kernels of the last call
    bool ran = false;
    float cpu_ms = 0.f;                 // CPU backend: wall time of the last call
};
enum { kSvcAov = 0, kSvcDenoise, kSvcReproject, kSvcPreview, kSvcNoise, kSvcDenoiseNoise, kSvcChain, kSvcCount };

struct bdpt_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    // Pass-stream folds (bdpt_accum_kernel) run on their own stream so that a launch's fold
    // overlaps the next launch's path kernel (VALU-bound; the fold is a memory stream); pixel
    // pools fold on `stream` right after their launch instead (bdpt_accum_serial_kernel).  The
    // radiance buffer is double-buffered: launch L writes half L % 2 after the fold of launch L-2
    // has read it.  Everything else that touches colors/counter/pixels runs on `stream` after
    // join_fold() has made it wait for the last concurrent fold.
    hipStream_t fstream = nullptr;
    // Pixel pools with overlapped launches: a pooled launch and its serial fold run on
    // pstream[half of the radiance buffer], so one launch's drain overlaps the next one's start;
    // the folds stay in order through rb_fold_ev.  Everything queued on `stream` that feeds or
    // follows the path kernels joins the last fold first (join_fold).
    hipStream_t pstream[2] = {nullptr, nullptr};
    hipEvent_t amark = nullptr;         // `stream`'s work before a call, for the pstreams to wait on
    bool pool_dirty = false;            // overlapped launches used the claim-counter sets
    unsigned long long* d_prof = nullptr;   // BDPT_PROF=1 (with a -DBDPT_PROF kernel): section cycles
    hipEvent_t rb_path_ev[2] = {nullptr, nullptr};   // path kernel of the half done (stream)
    hipEvent_t rb_fold_ev[2] = {nullptr, nullptr};   // fold of the half done (fstream)
    bool rb_used[2] = {false, false};
    int rb_next = 0, fold_last = 0;
    bool fold_pending = false;          // a fold was issued after the last join_fold
    hipStream_t fold_stream = nullptr;  // the stream of the last fold (fstream or a pstream)
    // Path-pass calls go through a ring of kRing slots, each with its own events, so a call
    // never waits for the GPU except on the call issued kRing calls earlier (the reference's
    // interactive loop issues one pass per call; the pass tables travel in the kernel
    // arguments).  Timing is folded lazily, in call order.
    static constexpr int kRing = 4;
    struct call_slot {
        hipEvent_t ev0 = nullptr, ev1 = nullptr;   // the whole call
        std::vector<hipEvent_t> kev;               // per path-kernel launch {before, after}
        int launches = 0;
        bool pending = false;                      // issued, not folded yet
        bool serial_fold = false;                  // its folds ran after its path kernels, in-stream
        std::vector<unsigned> tiles;               // a masked call's tile list while its upload may be pending
    } ring[kRing];
    long long issued = 0, folded = 0;   // calls issued / folded into the accumulators
    double acc_ms = 0.0;         // accumulated device time of finished path-pass calls
    long long acc_launches = 0;
    float last_ms = 0.f;
    double acc_kernel_ms = 0.0;    // path kernels alone (no fold kernel)
    int W = 0, H = 0;
    std::vector<bdpt_sphere> spheres;
    std::vector<int> lights;
    bdpt_camera cam{};
    bool cam_set = false;
    bool rand_ready = false;
    int shard = 0, nshards = 1, band_rows = 8;
    int streams_req = 0;                // bdpt_set_streams: 0 = auto (measured), -1 = one pass per lane
    // auto mode: the first ten calls of >= 2 passes each measure one kernel variant (roles 0..9,
    // the table in bdpt_plan.h); the eleventh decides which one later calls run.
    bdpt_tuner tuner;
    // multi-device groups: the peers follow the stream mode devices[0] measured (its decision is
    // copied when they reach the decision point), so every device of a group runs the same kernels
    bdpt_ctx* group_leader = nullptr;
    int last_streams = 1;               // S of the last path-pass launch
    bool last_bvh = false;              // the last path-pass launch traversed the BVH
    int cus = 256;                      // compute units (auto stream count)
    // LDS per workgroup the device allows (hipDeviceAttributeMaxSharedMemoryPerBlock), the static
    // LDS of the path kernels looked at so far (by function), and the figures of the last
    // bdpt_path_passes call's largest launch, refused or not (bdpt_path_lds)
    size_t lds_limit = 0;
    std::vector<std::pair<const void*, size_t>> lds_static;
    size_t last_lds_static = 0, last_lds_dynamic = 0;
    bdpt_dev_vec* d_rbuf = nullptr;     // pass-stream radiance, 2 halves of rbuf_cap: [npass][nloc]
    unsigned* d_rmask = nullptr;        // pixel pools: 4 words per launched pixel (stored passes), 2 halves
    unsigned* d_poolctr = nullptr;      // pixel pools: claimed pixels per pass and eighth, a line each,
                                        // two sets: a pooled launch uses one and zeroes the other
    int pool_set = 0;                   // the set the next pooled launch uses
    unsigned* d_uflags = nullptr;       // ordered in-kernel fold (units): per 8x8 wave tile, epoch << 8 | range
    size_t uflags_cap = 0;
    unsigned uepoch = 0;                // launches of the units kernel (flag tags)
    // bdpt_path_passes_tiles: the tile list of the last masked call (one buffer: a masked call joins
    // the outstanding fold, the list's other reader, before it uploads its own list on `stream`)
    unsigned* d_tiles = nullptr;
    size_t tiles_cap = 0;
    unsigned* d_uerr = nullptr;         // set by a unit whose handover wait timed out
    bool units_check = false;           // a units launch ran since the last error check
    int traversal = BDPT_TRAVERSE_AUTO; // bdpt_set_traversal
    bool has_bvh = false;               // the scene has a BVH (bdpt_bvh.cpp)
    int bvh_nn = 0, bvh_ns = 0, big_n = 0;
    float bvh_c[3] = {0.f, 0.f, 0.f}, bvh_r = 0.f, bvh_q = 0.f;
    float4 *d_bvh_nodes = nullptr, *d_bvh_geom = nullptr, *d_big_geom = nullptr, *d_mat = nullptr;
    int *d_bvh_ids = nullptr, *d_big_ids = nullptr;
    size_t rbuf_cap = 0;                // elements
    size_t rmask_lanes = 0;             // launched pixels the mask halves hold (4 words each)
    uint4* d_params = nullptr;          // 4096 x {matrix_a, mask_b, mask_c, seed}
    float* d_rand = nullptr;
    float* d_rndp = nullptr;            // planar copy of d_rand (bdpt_rand_planar_kernel)
    // Tables derived from d_rand that only some path kernels read: allocated on first need and
    // filled before the first launch of a kernel that reads them (ensure_scp / ensure_srec); every
    // table change (one_generate_rand: the light pass and a checkpoint load come through it) clears
    // the ready flags.  Each device of a multi-device context owns its own.
    float2* d_scp = nullptr;            // {sinf, cosf}(2 pi u) per d_rndp entry (bdpt_sincos_planar_kernel)
    float4* d_srec = nullptr;           // sample records (bdpt_sample_records_kernel, bdpt_device.h)
    bool scp_ready = false, srec_ready = false;   // they hold the current table's values
    bdpt_dev_lightpath* d_lp = nullptr;
    bdpt_dev_sphere* d_sph = nullptr;
    unsigned sph_cap = 0;
    int* d_lights = nullptr;
    float4* d_geom = nullptr;           // per sphere {p, rad^2}; then the n_vac non-emitters' (VLP-only shadow rounds)
    unsigned n_vac = 0;
    float4* d_lightrec = nullptr;       // per emitter {p, rad}, {e, (4*pi*rad)*rad}
    unsigned emis_mask = 0;
    bdpt_dev_vec* d_colors = nullptr;
    unsigned* d_counter = nullptr;
    uchar4* d_pixels = nullptr;
    float* d_thr = nullptr;
    uint32_t h_params[4 * BDPT_MT_RNG_COUNT];
    // scene-specialised path kernels (hipRTC), by compile options; modules live until destroy
    bool specialize = true;             // bdpt_set_specialize
    bool last_specialized = false;
    std::map<std::string, hipFunction_t> jit_fns;
    std::vector<hipModule_t> jit_mods;
    char jit_err[256] = {0};            // why the last specialisation fell back (diagnostics)
    int jit_waves = 0;                  // waves/SIMD bound of the last specialised build
    bool jit_zero_exit = false;         // the last specialised build has the black-surface exit
    // jit_path_kernel's answer per variant (bdpt_jit_variant::index) for the current scene and
    // specialise switch (jit_forget) and the environment it was built under (env, compared by
    // value): a call then resolves its kernel without rebuilding the option strings (tens of
    // microseconds per call, which the one-pass-per-call pattern pays every call)
    struct jit_memo_t {
        bool valid = false, zero_exit = false;
        hipFunction_t fn = nullptr;
        int waves = 0;
        bdpt_jit_env env;
        std::string err;
    } jit_memo[kJitVariants];
    int last_features = 0;              // BDPT_FEAT_* of the last path-pass launch
    unsigned rand_seed = 0;             // seed of the current MT607 table (rand_ready)
    bool rand_uploaded = false;         // the table came from bdpt_write_rand: it has no seed
    char err[512] = {0};
    // multi-device context (bdpt_create_multi): this context renders on devices[0] and owns the
    // peer contexts of the other devices; the frame is assembled on devices[0] by a sum-reduce
    bool multi = false;
    std::vector<bdpt_ctx*> peers;
    std::vector<void*> comms;           // ncclComm_t per device when the reduce runs on RCCL
    int reduce_mode = 0;                // kReduce*
    bool frame_stale = true;            // the assembled frame predates the last change
    bdpt_dev_vec* d_fcolors = nullptr;  // assembled frame (devices[0])
    unsigned* d_fcounter = nullptr;
    uchar4* d_fpixels = nullptr;
    bdpt_dev_vec* d_ftmp = nullptr;     // peer-copy staging (kReducePeer)
    unsigned* d_ftmpc = nullptr;
    char reduce_note[256] = {0};        // the RCCL version and communicator, or why RCCL is not used
    bdpt_cpu_ctx* cpu = nullptr;        // device == BDPT_DEVICE_CPU: the host backend (bdpt_cpu.cpp)
    hipGraphicsResource_t gl_res = nullptr;   // registered GL pixel-unpack buffer (bdpt_gl_register_pbo)
    // first-hit feature buffers (bdpt_render_aov): six output planes of aov_cap pixels each in one
    // allocation (12 words per pixel), made on the first call and grown when a window needs more
    float* d_aov = nullptr;
    size_t aov_cap = 0;
    int aov_traversal = 0;              // BDPT_TRAVERSE_* of the last bdpt_render_aov (0: none yet)
    // chain buffers (bdpt_render_chain): ten output planes of chain_cap pixels each in one allocation
    // (BDPT_CHAIN_WORDS words per pixel), made on the first call and grown when a window needs more
    float* d_chain = nullptr;
    size_t chain_cap = 0;
    // the frame services' clocks, by kSvc*: bdpt_render_aov (the kernel alone), bdpt_denoise,
    // capture / bdpt_reproject, bdpt_preview_denoise, bdpt_noise_estimate, bdpt_denoise_noise,
    // bdpt_render_chain (the kernel alone)
    bdpt_svc_clock svc[kSvcCount];
    // denoiser (bdpt_denoise): guide, ping and pong records of the whole frame in one allocation
    // (3 x 16 B per pixel), made on the first call -- the frame size never changes
    float4* d_dn = nullptr;
    // temporal reprojection (bdpt_reproject): two sets of {guide, colour + weight} records
    // (2 x 32 B per pixel; set hist_cur is the history, a capture writes the other) and the packed
    // results of a call (12 + 4 + 4 B per pixel) in one allocation, made on first use
    float4* d_hist = nullptr;
    int hist_cur = 0;
    bool has_hist = false;              // a history is stored (under hist_cam / hist_spheres)
    bdpt_camera hist_cam{};
    std::vector<bdpt_sphere> hist_spheres;
    // "follow" (bdpt_history_follow): the switch, and the spheres' offsets from hist_spheres as one
    // float4 per sphere on the device, made on first use; hdelta_up is what d_hdelta holds, so the
    // table is uploaded when the offsets change, not per call
    bool hist_follow = false;
    float4* d_hdelta = nullptr;
    std::vector<float4> hdelta_up;
    // (the denoised preview, bdpt_preview_denoise, works in d_dn and d_hist's result buffers)
    // noise estimate (bdpt_noise_estimate): the mark's 16-byte records and the results of a call
    // (the per-pixel plane, then S, E, c and the pending count per tile), each made on first use.
    // mark_live = false is the cleared mark: the kernel then reads every count as 0.
    uint4* d_mark = nullptr;
    bool mark_live = false;
    float* d_noise = nullptr;
    std::vector<unsigned> noise_pending;   // per tile, of the last estimate (bdpt_noise_tile_pending); empty: none yet
    unsigned gl_pbo = 0;
};
enum { kReduceNone = 0, kReduceRccl = 1, kReducePeer = 2 };

inline int fail(bdpt_ctx* c, int code, const char* fmt, ...) {
    if (c) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(c->err, sizeof(c->err), fmt, ap);
        va_end(ap);
    }
    return code;
}

#define HIPCHK(ctx, call)                                                                      \
    do {                                                                                       \
        hipError_t e_ = (call);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail((ctx), BDPT_EHIP, "%s: %s", #call, hipGetErrorString(e_));            \
    } while (0)

// Defined in bdpt_host.cpp, used by bdpt_frame.cpp and bdpt_jit.cpp too (hidden: not part of the
// library's exports).
namespace bdpt_host __attribute__((visibility("hidden"))) {
// Make the context's stream wait for the last fold: before anything on it touches colors / counter / pixels.
int join_fold(bdpt_ctx* c);
// The frame and camera constants of a launch, as the kernels take them.
void camera_args(const bdpt_ctx* c, const bdpt_camera& cam, bdpt_path_args& a);
// The BVH of the scene, for a launch that traverses it (without a.mat, which only the path kernels read).
void bvh_args(const bdpt_ctx* c, bdpt_path_args& a);
// After the stream has drained: BDPT_EHIP once if a units launch left the frame invalid.
int units_verdict(bdpt_ctx* c);
// The two planner switches (bdpt_path_env) that the specialised builds depend on as well:
// BDPT_UNITS at this moment, and BDPT_FUSED_MAX_PASSES as read once per process.
int units_env();
int fused_max_passes();

// Defined in bdpt_jit.cpp: the scene-specialised path kernels (what they build is in bdpt_jit_plan.h).
// The specialised kernel of a variant for the context's scene, compiled on first use; nullptr =
// the precompiled instance runs (reason in c->jit_err).  Sets c->jit_err / jit_waves / jit_zero_exit.
hipFunction_t jit_path_kernel(bdpt_ctx* c, const bdpt_jit_variant& v);
void jit_forget(bdpt_ctx* c);           // the scene or the specialise switch changed: resolve afresh
void jit_release(bdpt_ctx* c);          // unload the context's code objects (destroy)
bdpt_jit_env jit_env();                 // the builds' environment inputs, read now
bool jit_srec_enabled();                // jit_env().srec_enabled()
}  // namespace bdpt_host
