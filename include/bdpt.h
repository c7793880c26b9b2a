/*
 * bdpt.h -- C-ABI of the MI355X bidirectional path tracer (libbdpt.so).
 *
 * This is the drop-in boundary for the render path of sim186/gpu_bidirectional_raytracer.
 * In the reference the boundary is the set of module globals plus <<<>>> launches inside
 * src/smallpt_cpu.c; every entry point below names the reference function it replaces.
 * Plain C: no torch / HIP types in any signature.  All functions return 0 on success and a
 * negative BDPT_E* code on failure; the message is in bdpt_last_error() (the reference prints
 * cudaGetErrorString() and continues, smallpt_cpu.c:169-233 -- the host does the same with this).
 * One context per GPU; calls on one context must not run concurrently (the reference is single-
 * threaded too); different contexts are independent.
 *
 * Types are layout-compatible with the reference headers (static-asserted in the library):
 *   bdpt_vec       == Vec        include/vec.h:4-6       (12 B)
 *   bdpt_ray       == Ray        include/geom.h:9-11     (24 B)
 *   bdpt_sphere    == Sphere     include/geom.h:23-27    (44 B, enum Refl stored as int)
 *   bdpt_lightpath == LightPath  include/geom.h:29-33    (36 B)
 *   bdpt_camera    == Camera     include/camera.h:7-12   (60 B)
 */
#ifndef BDPT_H
#define BDPT_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct { float x, y, z; } bdpt_vec;
typedef struct { bdpt_vec o, d; } bdpt_ray;
enum { BDPT_DIFF = 0, BDPT_SPEC = 1, BDPT_REFR = 2, BDPT_LITE = 3 }; /* geom.h:18-20 enum Refl */
typedef struct { float rad; bdpt_vec p, e, c; int refl; } bdpt_sphere;
typedef struct { bdpt_vec hp, rad, nl; } bdpt_lightpath;
typedef struct { bdpt_vec orig, target, dir, x, y; } bdpt_camera;

/* Compile-time constants of the reference (cons.h, geom.h, smallpt_cpu.c:67-69). */
#define BDPT_MT_RNG_COUNT 4096              /* MersenneTwister.h:28                         */
#define BDPT_N_PER_RNG    1876              /* AlignUp(DivideRoundUp(7680000,4096),2)       */
#define BDPT_RAND_N       (4096 * 1876)     /* 7,684,096 floats = 30.7 MB                   */
#define BDPT_LIGHT_POINTS 4096              /* geom.h:15 LIGHT_POINTS (DEPTH=1, MAX_VLP=1)  */
#define BDPT_MAX_SEGMENTS 7                 /* device.cu:621 `depth > 6` break               */
#define BDPT_COUNTER_CAP  30000u            /* device.cu:607 `counter[i] < 30000`            */
#define BDPT_MAX_STREAMS  128               /* bdpt_set_streams upper bound                  */

/* Error codes. */
#define BDPT_OK        0
#define BDPT_EINVAL   -1   /* bad argument                                   */
#define BDPT_EIO      -2   /* file could not be read / written               */
#define BDPT_EHIP     -3   /* HIP runtime error                              */
#define BDPT_ENOMEM   -4   /* allocation failed                              */
#define BDPT_ESTATE   -5   /* call out of order (e.g. path pass before RNG)  */

typedef struct bdpt_ctx bdpt_ctx;

/* ---- render-path context (replaces smallpt_cpu.c module globals + AllocateBuffers) ---- */

/* AllocateBuffers smallpt_cpu.c:153-237 + loadMTGPU MersenneTwister_kernel.cu:23-36.
 * W,H are the internal sizes AFTER the reference's +1 (smallpt_cpu.c:409-410).
 * `device` is the HIP ordinal this context renders on, or BDPT_DEVICE_CPU for the host backend
 * (the smallpt_cpu.c CPU path: the same render path on the CPU cores, no GPU needed; identical
 * results; BDPT_CPU_THREADS sets its thread count).  Accumulation starts zeroed. */
#define BDPT_DEVICE_CPU (-1)
int  bdpt_create(bdpt_ctx **out, const bdpt_sphere *spheres, unsigned n_spheres,
                 int width, int height, const char *mt_dat_path, int device);
/* Multi-GPU context (SURVEY.md 8(b) `bdpt_create(..., devices, ndev)`; the reference renders on
 * one device, smallpt_cpu.c:422).  One sub-context per entry of devices[]: device k renders the
 * 8-row pixel bands (y / 8) % ndev == k, every other entry point below applies to all devices,
 * and the read-back entry points (bdpt_read_radiance / _pixels, bdpt_device_buffers,
 * bdpt_update_pixels) return the frame assembled on devices[0] by a sum-reduce: an in-process
 * RCCL ncclReduce over an ncclCommInitAll communicator when the devices are distinct, else peer
 * copies (several shards on one GPU, or BDPT_REDUCE=peer).  The result equals a one-device
 * context's bit for bit.  bdpt_set_shard(ctx, s, n, band) makes the whole group shard s of n
 * groups (multi-node).  bdpt_path_timing / bdpt_kernel_timing report the slowest device. */
int  bdpt_create_multi(bdpt_ctx **out, const bdpt_sphere *spheres, unsigned n_spheres,
                       int width, int height, const char *mt_dat_path, const int *devices, int ndev);
int  bdpt_num_devices(const bdpt_ctx *ctx);
/* "rccl", "peer", or "none" (a one-device context from bdpt_create). */
const char *bdpt_reduce_backend(const bdpt_ctx *ctx);
/* The frame reduce in words, into buf (at most cap bytes, NUL-terminated): for "rccl" the RCCL
 * version, the rank count ncclCommInitAll was given and the device list; for "peer" why RCCL
 * is not used.  Returns the full length, BDPT_EINVAL on bad arguments. */
int  bdpt_reduce_info(const bdpt_ctx *ctx, char *buf, int cap);
/* ncclGetVersion of the librccl this library binds to (e.g. 22606 = 2.26.6), BDPT_ESTATE if it
 * cannot be loaded.  Needs no GPU. */
int  bdpt_rccl_version(void);
/* Assemble the frame now (otherwise done on the first read-back after a change). */
int  bdpt_reduce_frame(bdpt_ctx *ctx);
/* FreeBuffers smallpt_cpu.c:98-110. */
void bdpt_destroy(bdpt_ctx *ctx);
const char *bdpt_last_error(const bdpt_ctx *ctx);
/* Message of the last failed bdpt_create (no context exists then). */
const char *bdpt_create_error(void);

/* ReInitScene smallpt_cpu.c:365-371 (re-upload of dev_spheres, :229). Does not run the light pass. */
int  bdpt_set_scene(bdpt_ctx *ctx, const bdpt_sphere *spheres, unsigned n_spheres);
/* Camera by value, as RadiancePathTracingKernel receives it (device.cu:548). Call after
 * bdpt_update_camera(). */
int  bdpt_set_camera(bdpt_ctx *ctx, const bdpt_camera *camera);
/* counter[] := 0 (ReInit -> AllocateBuffers, smallpt_cpu.c:204); colors/pixels follow on the
 * next pass because counter==0 assigns (device.cu:774). */
int  bdpt_reset_accum(bdpt_ctx *ctx);
/* Multi-GPU sharding: only pixels whose row band (y / band_rows) % nshards == shard are
 * rendered; all other pixels stay zero so a sum-reduce of the frames is exact. Default 0,1,8;
 * band_rows a multiple of 8 (the tile height) launches only the shard's own tile rows. */
int  bdpt_set_shard(bdpt_ctx *ctx, int shard, int nshards, int band_rows);
/* Pass streams (no reference counterpart; results are bit-identical for every S): S lanes per
 * pixel render passes s, s+S, ... into an HBM radiance buffer (12 B per pass and pixel) and an
 * ordered fold applies the running mean of device.cu:774-787 in pass order.
 *   0  = auto (default): the first ten calls of >= 2 passes measure, in this order, the
 *        pass-stream kernel with two passes per lane (S = ceil(passes / 2); one per lane in
 *        launches of < 4 passes or with the BVH), the fused kernel with paired segment loads,
 *        pass streams with four passes per lane (S = ceil(passes / 4), launches of >= 8), two
 *        per lane again, the fused kernel without pairing, four per lane again, twice pass
 *        streams with pixel pools (S = passes, lanes restart on new pixels of their pass;
 *        specialised builds, BDPT_FEAT_POOLS), and twice the ordered in-kernel fold (units of a
 *        tile and 8 passes, running mean in registers, no radiance buffer and no fold kernel;
 *        specialised builds of frames with >= 2 x CUs x 6 tile workgroups, BDPT_FEAT_UNITS);
 *        later calls use the pass-stream variant with the
 *        fastest call, or the faster fused variant if its time per pass (path kernels + a quarter of the fold) beat that by 5 %
 *        (closed scenes with long paths favour pass streams, open scenes with short paths the
 *        fused kernel or pools); re-measured after a scene / shard / traversal change;
 *  -1  = BDPT_STREAMS_PER_LANE: always one pass per lane (S = passes per launch, <= 128);
 *   1  = the fused kernel that keeps the running mean in registers (no buffer);
 *  2..128 = that many streams. */
#define BDPT_STREAMS_PER_LANE (-1)
int  bdpt_set_streams(bdpt_ctx *ctx, int streams);
/* S used by the last bdpt_path_passes call. */
int  bdpt_last_streams(const bdpt_ctx *ctx);
/* The kernel variant the auto stream mode settled on, as BDPT_CHOICE_* bits (0 while it is still
 * measuring, or when the stream mode is not auto).  bdpt_set_stream_choice applies such a choice
 * without measuring (every device of a group); a later scene / shard / traversal / stream-mode
 * change measures again.  No reference counterpart (smallpt_cpu.c:422 renders on one device): a
 * multi-GPU job lets one device measure and gives every device its choice, so all GPUs run the
 * same kernels -- the devices of a bdpt_create_multi group do this by themselves (they follow
 * devices[0]); torchrun ranks pass rank 0's choice along (bench.py). */
#define BDPT_CHOICE_DECIDED 1               /* a choice exists                                */
#define BDPT_CHOICE_FUSED   2               /* the fused S = 1 kernel                         */
#define BDPT_CHOICE_PAIRED  4               /* the fused variant with paired segment loads    */
#define BDPT_CHOICE_QUARTER 8               /* pass streams with four passes per lane         */
#define BDPT_CHOICE_POOLS  16               /* pass streams with pixel pools                  */
#define BDPT_CHOICE_UNITS  32               /* pass streams with the ordered in-kernel fold   */
int  bdpt_stream_choice(const bdpt_ctx *ctx);
int  bdpt_set_stream_choice(bdpt_ctx *ctx, int choice);
/* Device k of a (multi-device) context (0 = devices[0]): S and BDPT_FEAT_* bits of its last
 * bdpt_path_passes call, and its BDPT_CHOICE_* bits. */
int  bdpt_device_mode(bdpt_ctx *ctx, int k, int *last_streams, int *features, int *choice);
/* Scene-specialised kernels (no reference counterpart; results are bit-identical): for scenes of
 * <= 64 spheres (brute-force traversal) the path kernel is compiled at run time (hipRTC, ~1 s, cached on disk) with the
 * sphere geometry folded in as constants.  1 = on (default), 0 = precompiled kernels only.  If
 * hipRTC is unavailable or the compile fails, the precompiled kernel runs. */
int  bdpt_set_specialize(bdpt_ctx *ctx, int on);
/* 1 if the last bdpt_path_passes call ran a specialised kernel; the reason it did not, if not. */
int  bdpt_last_specialized(const bdpt_ctx *ctx);
const char *bdpt_specialize_status(const bdpt_ctx *ctx);
/* Sphere traversal (no reference counterpart; results are bit-identical either way).  The
 * reference tests every sphere per ray (IntersectDevice device.cu:106-124); for scenes with
 * > 16 spheres of which >= 24 are of ordinary size, bdpt_set_scene also builds a BVH over those
 * (walls stay brute force) that skips only spheres that provably cannot change the answer. */
#define BDPT_TRAVERSE_AUTO  0               /* BVH when it has >= 128 spheres                */
#define BDPT_TRAVERSE_BRUTE 1               /* every sphere, like the reference             */
#define BDPT_TRAVERSE_BVH   2               /* BVH whenever the scene has one               */
int  bdpt_set_traversal(bdpt_ctx *ctx, int mode);
int  bdpt_scene_has_bvh(const bdpt_ctx *ctx);
/* BDPT_TRAVERSE_BVH or BDPT_TRAVERSE_BRUTE: what the last bdpt_path_passes call used. */
int  bdpt_last_traversal(const bdpt_ctx *ctx);
/* What the kernel of the last bdpt_path_passes call compiled in (no reference counterpart; none of
 * these changes a result): bit flags below.  The three skips leave out work whose result the
 * reference computes and never uses, so a FLOP model priced on the reference's work counts more
 * than the kernel executes ("reference-equivalent" FLOPs). */
#define BDPT_FEAT_SPECIALIZED 1             /* scene-specialised build (hipRTC)              */
#define BDPT_FEAT_DET_SKIP    2             /* whole-wave skip of sphere tests all lanes miss */
#define BDPT_FEAT_ZERO_EXIT   4             /* paths end at a black non-emitter              */
#define BDPT_FEAT_LAST_SKIP   8             /* no next direction after the 7th segment        */
#define BDPT_FEAT_BVH        16             /* BVH traversal (large scenes)                   */
#define BDPT_FEAT_STREAMS    32             /* pass streams (one pass per lane + ordered fold)*/
#define BDPT_FEAT_POOLS      64             /* pass streams with pixel pools (lanes restart on
                                               new pixels of their pass, claimed in chunks)   */
#define BDPT_FEAT_SCP       256             /* sin/cos planes: the angles' sinf/cosf loaded, not
                                               evaluated (pass streams / units, not pools)     */
#define BDPT_FEAT_SREC      512             /* sample records: the cosine direction's coefficients
                                               and the NEE light sample of every table position
                                               loaded as one 32-B record, not computed per vertex
                                               (specialised pass streams / units; set with
                                               BDPT_FEAT_SCP, whose planes the records replace) */
#define BDPT_FEAT_UNITS     128             /* pass streams with the ordered fold in the kernel:
                                               units of (tile, range of passes) in range order,
                                               running mean in registers, no radiance buffer   */
#define BDPT_FEAT_TILES    1024             /* the launch enumerated a tile list: one workgroup per
                                               masked-in tile (bdpt_path_passes_tiles)         */
int  bdpt_last_kernel_features(const bdpt_ctx *ctx);
/* LDS of the last bdpt_path_passes call's largest launch, in bytes, whether it ran or was refused:
 * what the launched kernel declares itself (static), what the launch adds for the scene tables and
 * the staged passes (dynamic), and what the device allows a workgroup (limit).  A call whose
 * static + dynamic exceeds the limit fails with BDPT_EINVAL before anything is launched; such a
 * scene still renders with BDPT_TRAVERSE_BVH when it has a tree.  Zeros before the first call and
 * on the CPU backend.  Any pointer may be NULL. */
int  bdpt_path_lds(const bdpt_ctx *ctx, unsigned *static_bytes, unsigned *dynamic_bytes, unsigned *limit_bytes);
/* The black-surface exit rule (BDPT_FEAT_ZERO_EXIT): 1 if ending a path at a black non-emitter is
 * provably exact for this scene -- every term the reference adds after the black hit is finite,
 * so 0 * term = +0 leaves the radiance bit-identical -- else 0.  Pure host function: the
 * specialised build asks it, and tests check it against the Python restatement. */
int  bdpt_zero_exit_safe(const bdpt_sphere *spheres, unsigned n_spheres);

/* UpdateRendering2 smallpt_cpu.c:300-362: for every emitter in sphere order,
 * seedMTGPU(current_sample*5) + RandomGPU (MT607 table), GetRayKernel and
 * RadianceLightTracingKernel (4096 VLPs). */
int  bdpt_light_pass(bdpt_ctx *ctx, int current_sample);
/* Just the MT607 table: seedMTGPU(seed) + RandomGPU<<<32,128>>> (MersenneTwister_kernel.cu:39-110). */
int  bdpt_generate_rand(bdpt_ctx *ctx, unsigned seed);

/* `npass` x UpdateRendering (smallpt_cpu.c:265-297) fused into one launch: pass p uses
 * sid[p] (= rand()%RAND_N, :270) and vlp_index[p] (the :292-293 state machine).
 * Asynchronous on the context's stream (a call only waits for the call issued 4 calls earlier,
 * whose pass-table slot it reuses); bdpt_synchronize() waits for all. */
int  bdpt_path_passes(bdpt_ctx *ctx, const unsigned *sid, const int *vlp_index, int npass);
/* Path passes over some tiles only (no reference counterpart): the passes of
 * bdpt_path_passes for the pixels of the tiles whose byte in tile_mask is non-zero.  Tiles are the
 * noise estimate's: BDPT_NOISE_TW x BDPT_NOISE_TH pixels anchored at (0, 0), row-major, tiles_x *
 * tiles_y of them (bdpt_noise_tiles); tiles of the last column and row hold only their pixels inside
 * the frame.  A pixel of a masked-in tile gets exactly what bdpt_path_passes gives it -- the same
 * samples (sid and vlp_index are per pass, whatever the mask), the `counter < 30000` rule, the
 * pixel bytes; every other pixel keeps colours, counter and pixel bytes bit for bit.  Pixels are
 * independent, so a frame rendered under changing masks holds, per pixel, what the unmasked frame
 * held after as many passes as that pixel's tile was rendered for.
 *   tile_mask == NULL   is bdpt_path_passes: the same code path, auto stream mode included.
 *   all bytes zero      BDPT_OK after the usual argument and state checks; nothing is launched and
 *                       nothing changes (bdpt_kernel_timing's launch count included).
 * A masked call launches one workgroup per masked-in tile and pass stream (BDPT_FEAT_TILES) from a
 * tile list the context uploads before the launch.  It never runs pixel pools or the in-kernel fold
 * (BDPT_POOL / BDPT_UNITS are ignored) and it neither takes a turn of the auto stream mode's
 * measurement nor resets its decision: in auto mode it runs the variant kept (fused or pass
 * streams, two or four passes per lane), two passes per lane while there is no decision; explicit
 * bdpt_set_streams values are honoured.  Like any path pass it keeps the noise estimate's mark and
 * the reprojection history.  BDPT_EINVAL: a multi-device context or a sharded one (nshards > 1)
 * with a non-NULL mask, and what bdpt_path_passes refuses. */
int  bdpt_path_passes_tiles(bdpt_ctx *ctx, const unsigned *sid, const int *vlp_index, int npass,
                            const unsigned char *tile_mask);
int  bdpt_synchronize(bdpt_ctx *ctx);
/* *n = the path-pass calls the device has not finished yet: calls whose timing is not folded and
 * whose closing event has not fired (at most 4, the depth of the call ring; a multi-device context
 * sums its devices).  Read-only: it never waits, issues nothing and folds no timing, so a caller
 * can tell whether what it issues next is queued behind running passes.  0 on the CPU backend.
 * BDPT_EINVAL for a NULL argument. */
int  bdpt_calls_in_flight(bdpt_ctx *ctx, int *n);
/* Device time (ms, HIP events on the context's stream) of the last bdpt_path_passes call. */
int  bdpt_last_path_ms(bdpt_ctx *ctx, float *ms);
/* Accumulated device time and kernel-launch count of all path-pass calls since the last reset
 * (synchronises first).  reset != 0 zeroes the accumulators after reading them. */
int  bdpt_path_timing(bdpt_ctx *ctx, double *total_ms, long long *launches, int reset);
/* Same accumulation, but only the path kernels' own durations (one HIP event pair around each
 * path-kernel launch, excluding the pass-stream fold): what rocprof reports for that kernel.
 * Overlapped pooled launches (pixel pools, BDPT_FEAT_POOLS): consecutive launches run on two
 * streams and a launch starts while the previous one drains, so their event intervals overlap and
 * bdpt_last_path_ms, bdpt_path_timing and bdpt_kernel_timing add up to MORE than the wall time;
 * divide the wall time of a run by its launches for a per-launch rate (bench.py launch_overlap). */
int  bdpt_kernel_timing(bdpt_ctx *ctx, double *kernel_ms, long long *launches, int reset);
/* Device k of a (multi-device) context, 0 <= k < bdpt_num_devices (0 = devices[0]): its device
 * id (BDPT_DEVICE_CPU for the host backend), its own path-kernel ms and path ms (with the fold)
 * and launches since the last timing reset, and the pixels its shard owns.  Does not reset.
 * New (the reference is single-device, smallpt_cpu.c:422): lets a multi-GPU run report each
 * device's share instead of only the slowest. */
int  bdpt_device_timing(bdpt_ctx *ctx, int k, int *device, double *kernel_ms, double *path_ms,
                        long long *launches, long long *owned_pixels);

/* Read-back.  colors/counter: the float parity artefact (dev_colors / dev_counter);
 * pixels: uchar4 RGBA = pixels_buf (SavePPM, smallpt_cpu.c:241). */
int  bdpt_read_radiance(bdpt_ctx *ctx, bdpt_vec *colors, unsigned *counter);
int  bdpt_read_pixels(bdpt_ctx *ctx, unsigned char *rgba);
int  bdpt_read_rand(bdpt_ctx *ctx, float *rand_table);          /* d_Rand, BDPT_RAND_N */
/* Upload all BDPT_RAND_N entries of d_Rand (the counterpart of bdpt_read_rand; no reference
 * counterpart): tests render on tables no seed produces -- all zeros, one constant.  Ordered after
 * what is queued.  Such a table has no seed: until a table is generated again bdpt_rand_seed answers
 * BDPT_ESTATE, and a checkpoint saved meanwhile holds no table.  One-device contexts only. */
int  bdpt_write_rand(bdpt_ctx *ctx, const float *rand_table);
int  bdpt_read_lightpaths(bdpt_ctx *ctx, bdpt_lightpath *lp);   /* dev_lp, 4096        */
/* The sample records of the current table (BDPT_FEAT_SREC), built first if they are not current:
 * 8 floats per table position j < BDPT_RAND_N - 5, {A, B, C, u2, X, Y, Z, u0} of d_Rand[j..j+4]
 * (csrc/bdpt_math.h bdpt_sample_record), in table order -- 8 * (BDPT_RAND_N - 5) floats.  Tests. */
int  bdpt_read_sample_records(bdpt_ctx *ctx, float *records);
/* Upload all 4096 VLPs (the counterpart of bdpt_read_lightpaths; checkpoint restore). */
int  bdpt_write_lightpaths(bdpt_ctx *ctx, const bdpt_lightpath *lp);
/* The seed of the current MT607 table (current_sample * 5 of the last light pass, or the
 * bdpt_generate_rand argument); BDPT_ESTATE before any table exists. */
int  bdpt_rand_seed(const bdpt_ctx *ctx, unsigned *seed);
/* The context's camera (BDPT_ESTATE if none was set) and scene: bdpt_get_scene copies at most
 * `cap` spheres and returns the scene's sphere count (spheres may be NULL to ask the count). */
int  bdpt_get_camera(const bdpt_ctx *ctx, bdpt_camera *camera);
/* The frame size the context was created with (internal W, H). */
int  bdpt_frame_size(const bdpt_ctx *ctx, int *width, int *height);
int  bdpt_get_scene(const bdpt_ctx *ctx, bdpt_sphere *spheres, unsigned cap);
/* Device pointers for zero-copy collectives (RCCL reduce of the radiance frame).  Path passes
 * run asynchronously on the context's own stream: bdpt_synchronize() before using them.  For a
 * multi-device context: the assembled frame on devices[0]. */
int  bdpt_device_buffers(bdpt_ctx *ctx, void **colors, void **counter, void **pixels);
/* Recompute pixels (toInt gamma) from colors on the device, e.g. after a cross-GPU reduce. */
int  bdpt_update_pixels(bdpt_ctx *ctx);

/* ---- first-hit feature buffers (AOVs) and sphere picking (no reference counterpart: the
 * reference selects a sphere only by cycling '+'/'-', display_func.c:336-343) ----
 * The first segment of the eye path on its own, in the path kernel's arithmetic, for the pixels
 * (x, y) of the window [x0, x0+w) x [y0, y0+h) of the context's frame; outputs are packed [h][w].
 *   ray    the camera ray of device.cu:562-600 with the jitter randoms d_Rand[kk], d_Rand[kk+1],
 *          kk = (26 + 25*i + sid) % (RAND_N-5) (:562, 32-bit unsigned arithmetic), i = y*W + x the
 *          full-frame pixel index of bdpt_read_radiance -- so a window equals the same slice of
 *          the whole frame; jitter == 0: both randoms are +0.0f (no random table needed)
 *   hit    IntersectDevice device.cu:106-124 (downward scan, strict `<`, EPSILON rule of :80-104);
 *          the material plays no part: glass, mirrors and emitters are hits like any other
 *   id     sphere index, -1 on a miss
 *   t      hit distance along the normalised direction
 *   position  hitPoint, device.cu:635-637
 *   normal    the geometric normal of :639-641 (not flipped towards the ray)
 *   dp        vdot(normal, ray.d) of :643, signed: negative = the sphere is seen from outside
 *   dir       the normalised ray direction (also on a miss)
 * On a miss t, dp, position and normal are +0.0f.  Pointers are host memory; NULL = not wanted.
 * Synchronous, ordered after whatever the context has in flight, and without side effects: the
 * accumulation, counters, pixels, random tables, VLPs, path timing, stream and kernel choices and
 * shards are untouched, so passes rendered after the call equal passes rendered without it.
 * bdpt_set_traversal is honoured -- BDPT_TRAVERSE_AUTO here means the BVH whenever the scene has
 * one -- with the same result either way (on the BVH equal distances go to the higher index).
 * BDPT_ESTATE: no camera set, or jitter != 0 before a random table exists.  BDPT_EINVAL: NULL
 * `out`, an empty window or one outside the frame, sid >= BDPT_RAND_N, or a multi-device context
 * (bdpt_create_multi): feature buffers are rendered by one-device contexts only. */
typedef struct { int *id; float *t; float *dp; bdpt_vec *position, *normal, *dir; } bdpt_aov_buffers;
int  bdpt_render_aov(bdpt_ctx *ctx, int x0, int y0, int w, int h, int jitter, unsigned sid,
                     const bdpt_aov_buffers *out);
/* The 1x1 window at (x, y): which sphere the pixel shows (-1: none) and how far away it is. */
int  bdpt_pick(bdpt_ctx *ctx, int x, int y, int jitter, unsigned sid, int *id, float *t);
/* Of the last bdpt_render_aov / bdpt_pick call: BDPT_TRAVERSE_BVH or BDPT_TRAVERSE_BRUTE, and the
 * device time of its kernel alone (ms, HIP events around the launch, no read-back; wall time of
 * the loop on the CPU backend).  BDPT_ESTATE before the first call. */
int  bdpt_last_aov_traversal(const bdpt_ctx *ctx);
int  bdpt_last_aov_ms(bdpt_ctx *ctx, float *ms);

/* ---- chain buffers: the eye path up to its first non-specular vertex (no reference counterpart;
 * DESIGN.md 4j) ----
 * What a pixel shows through mirrors and glass: the integrator follows a mirror deterministically and
 * glass by one random number, and stops being a chain at the first diffuse surface, emitter or miss
 * (device.cu:621-771).  Window, `jitter`, `sid`, traversal, outputs packed [h][w], NULL = not wanted,
 * "synchronous, ordered after what is queued, no side effects": all as bdpt_render_aov.  fp32, no
 * contraction, correctly rounded sqrt and divide, denormals kept, in the order written; vnorm(v) =
 * (1.f / sqrtf((v.x*v.x + v.y*v.y) + v.z*v.z)) * v; the GPU, the CPU backend and the tests' numpy
 * statement form the same bits.
 *   ray     bdpt_render_aov's: o, d.  thr = (1, 1, 1), len = +0, bounces = 0.
 *   loop    depth = 0 .. 6 (:621), j = (26 + 25*i + 5*depth + sid) % (RAND_N-5) (:619, 32-bit unsigned).
 *     hit     as bdpt_render_aov's (IntersectDevice :106-124); depth 0's sphere index is first_id
 *             (-1 on a miss).  A miss: kind = MISS, stop.
 *     vertex  len = len + t;  P = o + t*d (:635-637);  N = vnorm(P - p[s]) (:639-641);
 *             dp = vdot(N, d) (:643);  nl = dp > 0 ? -N : N (:645-647).
 *     stop    e[s] not all zero: kind = EMITTER, id = s, stop (:651, before the material).
 *             refl[s] == DIFF: kind = DIFFUSE, id = s, stop (:663).
 *     mirror  otherwise bounces += 1, R = d - (2.f * vdot(N, d)) * N, o = P.
 *             refl[s] == SPEC (:704-714): thr = thr * c[s], d = R, next depth.
 *     glass   any other refl (:715-770): into = vdot(N, nl) > 0;  nnt = into ? 1.f/1.5f : 1.5f/1.f;
 *             ddn = vdot(d, nl);  cos2t = 1.f - nnt*nnt*(1.f - ddn*ddn).
 *             cos2t < 0 (total internal reflection): thr = thr * c[s], d = R, next depth.
 *             td = vnorm(nnt*d - ((into ? 1.f : -1.f) * (ddn*nnt + sqrtf(cos2t))) * N);
 *             R0 = (0.5f*0.5f) / (2.5f*2.5f);  cc = 1 - (into ? -ddn : vdot(td, N));
 *             Re = R0 + (1 - R0)*cc*cc*cc*cc*cc (left to right);  Tr = 1.f - Re;  P = .25f + .5f*Re;
 *             RP = Re / P;  TP = Tr / (1.f - P).
 *             BDPT_CHAIN_TRANSMIT: thr = (TP * thr) * c[s], d = td.
 *             BDPT_CHAIN_PASS: d_Rand[j+2] < P ? (thr = (RP * thr) * c[s], d = R)
 *                                              : (thr = (TP * thr) * c[s], d = td)  -- what pass `sid` does.
 *     Leaving the loop after depth 6: kind = EXHAUSTED.
 *   id        the end sphere (DIFFUSE, EMITTER), -1 for MISS and EXHAUSTED
 *   first_id  bdpt_render_aov's id
 *   kind      BDPT_CHAIN_KIND_*
 *   bounces   mirror and glass vertices passed, 0..7
 *   t         len: the summed distances of the segments that hit
 *   dp, position, normal   of the end vertex (dp signed, the normal not flipped); +0.0f for MISS and
 *             EXHAUSTED
 *   dir       d when the loop is left: the direction of the segment that reached the end vertex or
 *             missed; for EXHAUSTED the direction the 7th vertex sends the path on in
 *   throughput  thr
 * Where bounces == 0 the six planes shared with bdpt_render_aov equal its planes.  With probe emitters
 * on the non-specular spheres and a zero light-path table, one path pass returns, per channel,
 * throughput * (fabsf(dp) * e[id]) of the BDPT_CHAIN_PASS chain: the pin the tests hold it to.
 * BDPT_EINVAL: an unknown `branch`, BDPT_CHAIN_PASS with jitter == 0 (the choice is a pass's), and
 * what bdpt_render_aov refuses, the multi-device context included.  BDPT_ESTATE as bdpt_render_aov.
 * bdpt_last_chain_ms: the device time of the last call's kernel alone (HIP events around the launch;
 * wall time of the loop on the CPU backend), BDPT_ESTATE before the first call. */
#define BDPT_CHAIN_TRANSMIT 0   /* glass: refract whenever refraction exists (no table needed) */
#define BDPT_CHAIN_PASS     1   /* glass: the choice pass `sid` makes, rnd[j+2] < P (needs jitter != 0) */
#define BDPT_CHAIN_KIND_DIFFUSE   0
#define BDPT_CHAIN_KIND_EMITTER   1
#define BDPT_CHAIN_KIND_MISS      2
#define BDPT_CHAIN_KIND_EXHAUSTED 3
typedef struct { int *id, *first_id, *kind, *bounces; float *t, *dp;
                 bdpt_vec *position, *normal, *dir, *throughput; } bdpt_chain_buffers;
int  bdpt_render_chain(bdpt_ctx *ctx, int x0, int y0, int w, int h, int jitter, unsigned sid,
                       int branch, const bdpt_chain_buffers *out);
int  bdpt_last_chain_ms(bdpt_ctx *ctx, float *ms);

/* ---- edge-avoiding wavelet denoiser guided by the first-hit buffers (no reference counterpart:
 * the reference shows and saves only the raw running mean, smallpt_cpu.c:239-262) ----
 * An a-trous filter over the context's accumulated radiance (what bdpt_read_radiance returns) as
 * it stands when the call runs, after whatever is queued on the context.  Guides: id and normal of
 * the unjittered first hit (bdpt_render_aov with jitter = 0, whole frame).  Pixel (x, y) is frame
 * index y*W + x.  fp32, no contraction, in the order written; the GPU, the CPU backend and the
 * tests' numpy statement form the same bits.
 *   eligible   BDPT_DENOISE_DIFFUSE: id >= 0 and spheres[id].refl == BDPT_DIFF; BDPT_DENOISE_ALL:
 *              id >= 0.  Ineligible pixels (misses; by default mirrors, glass, LITE emitters, whose
 *              first hit says nothing about what they show) are copied through at every level.
 *   level k    = 0 .. levels-1, step s = 2^k, h = (1/16, 1/4, 3/8, 1/4, 1/16),
 *              isc_k = (1.0f / (sigma_color * sigma_color)) * (float)4^k.  For an eligible centre p:
 *              sw = +0, sc = (+0, +0, +0); for j = 0..4 (dy = (j-2) s), for i = 0..4 (dx = (i-2) s),
 *              a tap q inside the frame with id[q] == id[p] adds
 *                d  = (n_p.x*n_q.x + n_p.y*n_q.y) + n_p.z*n_q.z
 *                wn = max(d, 0), then wn = wn*wn normal_power times
 *                dc = cur[q] - cur[p];  e2 = (dc.x*dc.x + dc.y*dc.y) + dc.z*dc.z
 *                wc = 1 / (1 + e2*isc_k);  w = ((h[j]*h[i]) * wn) * wc
 *                sw = sw + w;  sc = sc + w*cur[q]
 *              and out = sc * (1/sw) (both divisions correctly rounded).  Level k+1 reads level k.
 *              Denormal intermediates are kept, not flushed; non-finite radiance is not special.
 *   through    BDPT_DENOISE_THROUGH (bdpt_denoise and bdpt_denoise_noise only): the guides come from
 *              bdpt_render_chain with jitter = 0, BDPT_CHAIN_TRANSMIT, whole frame, instead of the
 *              first hit.  A pixel is eligible iff kind == DIFFUSE; its guide normal is the end
 *              normal; its guide integer -- what "id" means in the level (and in bdpt_denoise_noise's
 *              prefilter) -- is the key: id where bounces == 0, otherwise
 *              n + ((bounces-1)*n + first_id)*n + id with n the sphere count, so two pixels match when
 *              they show the same sphere through the same first sphere in as many bounces.  Nothing
 *              else of the filter changes.  A scene with 6 n*n + n > 2^31 - 1 is BDPT_EINVAL for this
 *              value only.  bdpt_reproject, bdpt_history_capture and bdpt_preview_denoise refuse it.
 *   levels 1..8, normal_power 0..6, sigma_color > 0 (+inf: no colour stopping).
 * colors_out: W*H denoised colours; rgba_out: 4*W*H bytes, the denoised frame through the toInt
 * thresholds and alpha of bdpt_read_pixels.  Either may be NULL, not both.  Synchronous; writes
 * nothing but its own buffers: accumulation, counters, pixels, tables, VLPs, path timing, the auto
 * stream mode's measurements and shards are untouched.  It filters the frame buffer as it stands:
 * a sharded caller uploads the assembled frame with bdpt_write_radiance first.
 * BDPT_EINVAL: NULL or out-of-range parameters, both outputs NULL, or a multi-device context
 * (bdpt_create_multi).  BDPT_ESTATE: no camera set. */
#define BDPT_DENOISE_DIFFUSE 0
#define BDPT_DENOISE_ALL     1
#define BDPT_DENOISE_THROUGH 3   /* guides through mirrors and glass (bdpt_render_chain); 2 is no
                                    value: callers that probe the field with it keep their BDPT_EINVAL */
typedef struct { int levels; int normal_power; float sigma_color; int materials; } bdpt_denoise_params;
int  bdpt_denoise(bdpt_ctx *ctx, const bdpt_denoise_params *params, bdpt_vec *colors_out,
                  unsigned char *rgba_out);
/* Device time (ms) of the last bdpt_denoise call's kernels alone (HIP events around the guide, pack
 * and level launches, no read-back; wall time on the CPU backend).  BDPT_ESTATE before any call. */
int  bdpt_last_denoise_ms(bdpt_ctx *ctx, float *ms);

/* ---- temporal reprojection: the last view's frame in the preview after a camera move (no
 * reference counterpart: every camera key goes through ReInit, smallpt_cpu.c:373-387, which
 * discards the frame) ----
 * A preview only: nothing here feeds back into the accumulation or the counters.  fp32, no
 * contraction, in the order written; dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z; every 1/x is the
 * correctly rounded reciprocal; denormals are kept; non-finite radiance is not special.  The GPU,
 * the CPU backend and the tests' numpy statement form the same bits.
 *   history   a context-owned snapshot taken under a camera C0 and the sphere array of that
 *             moment.  Per pixel q: a colour hc[q], a weight hm[q] >= 0 (the float count of passes
 *             behind the colour) and the guides gid[q], gpos[q] = id and position of
 *             bdpt_render_aov with jitter = 0 under C0, whole frame, rendered once when the history
 *             is taken.  While the context's spheres differ from the remembered array byte for
 *             byte the history counts as absent (a moved sphere changes the lighting everywhere;
 *             "follow" below is the opt-in exception).
 *   C0        as the kernels' camera constants: ux, uy, ud = vnorm of C0.x, C0.y, C0.dir
 *             (l = 1.f / sqrtf((x*x + y*y) + z*z), each component times l); o = C0.orig;
 *             inv_w = (float)(14./W), inv_h = (float)(10.5/H);
 *             hw = (float)((double)(inv_w*(float)W)/2.), hh likewise; sx = 1.f/inv_w, sy = 1.f/inv_h.
 *   pixel p = (x, y): c = colors[p], n = (float)counter[p] as they stand; id1, t1, P, N = id, t,
 *             position, normal of the current camera's unjittered first hit.
 *    1. m = 0 when no history is present, id1 < 0, or p is not eligible (materials ==
 *       BDPT_DENOISE_DIFFUSE: spheres[id1].refl == BDPT_DIFF; BDPT_DENOISE_ALL: any hit).
 *    2. v = P - o; a = dot(v, ux); b = dot(v, uy); cz = dot(v, ud); r = 1/cz;
 *       kx = (10.f*a)*r; ky = (10.f*b)*r; fx = (kx + hw)*sx; fy = (ky + hh)*sy.
 *       Unless fx >= -1 && fx < W && fy >= -1 && fy < H (a NaN fails): m = 0.
 *    3. x0 = floorf(fx), wx = fx - x0, y0 = floorf(fy), wy = fy - y0; sw = sm = +0, sc = (+0,+0,+0);
 *       for dy = 0, 1, for dx = 0, 1: q = (x0+dx, y0+dy), bx = dx ? wx : 1.f - wx,
 *       by = dy ? wy : 1.f - wy, bw = bx*by.  The tap is used iff q is inside the frame, bw > 0,
 *       gid[q] == id1, hm[q] > 0 and fabsf(dot(gpos[q] - P, N)) <= plane_tol * t1; a used tap adds
 *       sw = sw + bw; sm = sm + bw*fminf(hm[q], max_history); sc = sc + bw*hc[q].  A tap that is
 *       not used is skipped, not weighted by zero.
 *    4. No tap used: m = 0.  Otherwise h = sc*(1/sw), m = sm.
 *    5. tot = n + m; out = c if m == 0 (unchanged, and stale if n == 0, exactly what
 *       bdpt_read_radiance returns); out = h if n == 0 and m > 0; else out = (n*c + m*h)*(1/tot);
 *       weight_out = tot.
 * The id test rejects a point the old view did not show, the plane test one on the far side of the
 * same sphere.  Defaults: materials DIFFUSE, max_history 64, plane_tol 0.01.
 *
 * bdpt_history_capture forms (out, weight_out) as above from the history present, if any (without
 * one: colors and (float)counter), stores them as the new hc, hm with the current camera as C0, the
 * current spheres as the key and the guides rendered under the current camera; the records are
 * ping-ponged, so the capture reads the old history while it writes the new one.  Call it before
 * the camera changes.  bdpt_history_write uploads a history from the host and renders its guides
 * under `camera` and the current scene.  bdpt_history_info: *present is 0 also while the scene
 * differs; *camera is C0 (written only when a history is stored).  bdpt_history_read: the stored
 * colours and weights (also while the scene differs), BDPT_ESTATE when none is stored.  bdpt_reproject without a history present is
 * valid and returns colors and (float)counter; rgba_out goes through the toInt thresholds and alpha
 * of bdpt_read_pixels; any output may be NULL, not all.  bdpt_last_reproject_ms: device time of the
 * last capture's or reprojection's kernels alone (HIP events; wall time on the CPU backend).
 * All are synchronous, ordered after whatever the context has queued, and write nothing but the
 * history and their own buffers: accumulation, counters, pixels, tables, VLPs, path timing, the auto
 * stream mode's measurements and shards are untouched.  The history is not part of a checkpoint.
 * BDPT_EINVAL: NULL parameters or all outputs NULL, materials outside 0 and 1, max_history not > 0
 * (NaN rejected, +inf allowed), plane_tol negative or NaN (+inf: no plane test), a multi-device
 * context.  BDPT_ESTATE: no camera set (bdpt_reproject, bdpt_history_capture);
 * bdpt_last_reproject_ms before the first successful call. */
typedef struct { int materials; float max_history; float plane_tol; } bdpt_reproject_params;
int  bdpt_history_capture(bdpt_ctx *ctx, const bdpt_reproject_params *params);
int  bdpt_history_clear(bdpt_ctx *ctx);
int  bdpt_history_info(const bdpt_ctx *ctx, int *present, bdpt_camera *camera);
int  bdpt_history_read(bdpt_ctx *ctx, bdpt_vec *colors, float *weight);
int  bdpt_history_write(bdpt_ctx *ctx, const bdpt_camera *camera, const bdpt_vec *colors,
                        const float *weight);
int  bdpt_reproject(bdpt_ctx *ctx, const bdpt_reproject_params *params, bdpt_vec *colors_out,
                    float *weight_out, unsigned char *rgba_out);
int  bdpt_last_reproject_ms(bdpt_ctx *ctx, float *ms);

/* ---- "follow": the history stays usable when a sphere is moved (no reference counterpart: every
 * sphere key goes through ReInitScene, smallpt_cpu.c:365-371, which discards the frame;
 * DESIGN.md 4k) ----
 * Opt-in.  A moved sphere does change the lighting everywhere, but at preview sample counts the
 * noise of a fresh frame is far larger than the bias of the stale shadows, and nearly all of the
 * old frame is still the same surface: with follow on, a history taken under the spheres S0 stays
 * present under the spheres S when S differs from S0 only by translations of non-emitting spheres,
 * and a pixel that shows a moved sphere fetches its history where that sphere was.
 *   state     of the stored history against the context's spheres (bdpt_history_motion):
 *               BDPT_HISTORY_NONE     0  no history stored
 *               BDPT_HISTORY_SAME     1  stored, and the spheres are equal byte for byte
 *               BDPT_HISTORY_MOVED    2  stored and followable
 *               BDPT_HISTORY_UNUSABLE 3  stored and not usable
 *   followable  the sphere count is the same; for every k rad, e, c and refl are byte-equal; p may
 *             differ only where all three components of e compare == 0.f (the rule by which the
 *             path kernel's light list is filled).  A moved emitter, a changed radius, colour or
 *             material and a changed count make the history absent, as without follow.
 *   delta[k]  = S[k].p - S0[k].p, per component, in fp32, formed on the host; +0 where the
 *             components compare equal.
 *   bdpt_reproject with follow on: in state 1 as defined above; in state 2 as defined above with
 *             one change: P' = P - delta[id1] (per component, fp32) replaces P in step 2 (v = P' - o)
 *             and in the plane test of step 3 (fabsf(dot(gpos[q] - P', N)) <= plane_tol * t1).
 *             id1, t1, N, the eligibility rule, the tap order, the cap and the blend are untouched;
 *             the id test already refuses taps on what the sphere used to hide.  x - (+0) == x for
 *             every x, -0 included (-0 - (+0) = -0), so a pixel on an unmoved sphere forms the bits
 *             of the definition above.  bdpt_history_info reports present = 1 in state 2 while
 *             follow is on.
 *   bdpt_history_capture in state 2 with follow on forms (out, weight_out) as just defined and
 *             stores them with the current camera as C0 and the current spheres as the key: the
 *             state becomes 1, and captures chain across sphere moves as they do across camera
 *             moves (a camera move and a sphere move between two captures need nothing more: C0
 *             and delta are independent).  bdpt_preview_denoise takes bdpt_reproject's output
 *             exactly as defined there, so it follows without a parameter of its own.
 * bdpt_history_follow: the switch, off by default; it belongs to the context and survives
 * bdpt_set_scene, bdpt_set_camera and bdpt_reset_accum.  While it is off every call answers as
 * without this section: the same bits, the same `present`, the same errors.  bdpt_history_motion:
 * *state as above, whether follow is on or off; in states 1 and 2 delta[0..n) takes the offsets (all
 * +0 in state 1), otherwise it is left alone.  delta may be NULL; otherwise n must equal the
 * context's sphere count.  state may be NULL.
 * BDPT_EINVAL: a NULL or multi-device context, delta with n other than the sphere count. */
enum { BDPT_HISTORY_NONE = 0, BDPT_HISTORY_SAME = 1, BDPT_HISTORY_MOVED = 2, BDPT_HISTORY_UNUSABLE = 3 };
int  bdpt_history_follow(bdpt_ctx *ctx, int on);
int  bdpt_history_motion(const bdpt_ctx *ctx, int *state, bdpt_vec *delta, unsigned n);

/* ---- the reprojected preview, denoised with per-pixel sample counts (no reference counterpart;
 * DESIGN.md 4f) ----
 * One call: the reprojected frame in, the filtered frame out.  An a-trous filter as bdpt_denoise's
 * in which every record carries a sample count: a tap is weighted by its count, and the colour
 * stopping is scaled by how much the two counts say the pixels may differ.  fp32, no contraction,
 * in the order written; dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z; 1/x is the correctly rounded
 * reciprocal and a / b the correctly rounded IEEE division; denormals are kept; a tap that is not
 * used is skipped, not weighted by zero.  The GPU, the CPU backend and the tests' numpy statement
 * form the same bits.
 *   input     (o[p], tot[p]) = out and weight_out of bdpt_reproject under rp, exactly as defined
 *             there, from the history present or none.
 *   guides    id[p], n[p]: the unjittered first hit under the current camera, as for bdpt_denoise.
 *   eligible  as for bdpt_denoise with materials = rp.materials (one setting for both stages).
 *   levels == 0   colors_out = o, weight_out = tot, rgba_out = the RGBA of o: bit for bit the
 *             outputs of bdpt_reproject.
 *   clamp     for levels >= 1 a record's count is a = clampc(W): 0 when W == 0, otherwise
 *             fminf(fmaxf(W, 0x1p-20f), 0x1p40f).  It is applied when a record is written: at entry
 *             to tot, and to every level's output count.  a_p*a_q and a_p + a_q then stay inside
 *             [2^-40, 2^80], so absurd uploaded weights or max_history = +inf cannot form 0*inf.
 *   level k   = 0 .. levels-1, step s = 2^k, h and isc_k as for bdpt_denoise, c2 = 2.f / count_ref.
 *             An ineligible pixel is copied through, colour and count.  For an eligible centre p:
 *             su = sw = +0, sc = (+0, +0, +0); for j = 0..4 (rows, outer), for i = 0..4 (columns), a
 *             tap q is used iff it is inside the frame, id[q] == id[p] and a_q > 0; a used tap adds
 *               d  = dot(n_p, n_q);  wn = max(d, 0), then wn = wn*wn normal_power times
 *               dc = cur[q] - cur[p];  e2 = dot(dc, dc)
 *               g  = ((a_p*a_q) * (1/(a_p + a_q))) * c2;  wc = 1 / (1 + (e2*isc_k)*g)
 *                    (a_p == 0: wc = 1.f; the centre itself is then not a used tap)
 *               u  = ((h[j]*h[i]) * wn) * wc;  w = u * a_q
 *               su = su + u;  sw = sw + w;  sc = sc + w*cur[q]
 *             No tap used: out = cur[p], count a_p (= 0).  Otherwise out = sc * (1/sw) and the new
 *             count is clampc(sw / su).  Level k+1 reads level k's colours and counts.
 * Why: a_q-weighting is the inverse-variance combination of means of a_q samples; two pixels of one
 * true colour differ with variance proportional to 1/a_p + 1/a_q, hence the stopping term scaled by
 * a_p*a_q/(a_p + a_q), normalised so that two pixels of count_ref passes each give g == 1; the
 * carried count is the u-weighted mean count (never more than a tap had); sw / su is a true
 * division so that uniform counts stay exactly uniform -- with 8 passes everywhere, no history and
 * count_ref = 8 the call returns bdpt_denoise's bits.
 *   levels 0..8, normal_power 0..6, sigma_color > 0 (+inf allowed), count_ref > 0 and finite, rp as
 *   bdpt_reproject checks it.  Defaults: levels 4, normal_power 5, sigma_color 0.5, count_ref 8.
 * colors_out, weight_out: W*H of the last level; rgba_out through the toInt thresholds and alpha of
 * bdpt_read_pixels.  Any may be NULL, not all.  Synchronous, ordered after whatever is queued, and
 * like bdpt_reproject it writes nothing but its own buffers: the history, accumulation, counters,
 * pixels, tables, VLPs, path timing, the auto stream mode's measurements and shards are untouched.
 * BDPT_EINVAL: anything out of range, all outputs NULL, a multi-device context.  BDPT_ESTATE: no
 * camera set.  bdpt_last_preview_ms: device time of the last successful call's kernels alone (HIP
 * events; wall time on the CPU backend), BDPT_ESTATE before the first. */
typedef struct { bdpt_reproject_params rp; int levels; int normal_power;
                 float sigma_color; float count_ref; } bdpt_preview_params;
int  bdpt_preview_denoise(bdpt_ctx *ctx, const bdpt_preview_params *params, bdpt_vec *colors_out,
                          float *weight_out, unsigned char *rgba_out);
int  bdpt_last_preview_ms(bdpt_ctx *ctx, float *ms);

/* ---- per-tile noise estimate from two frames (no reference counterpart) ----
 * How noisy the frame is, so that a caller can stop when it is good enough.  The path kernel keeps
 * no sum of squares; the estimate is the half-buffer one: a context-owned mark holds the frame as
 * it stood some passes ago, and how far the running mean has moved since, scaled by the two sample
 * counts, estimates the error of the present mean.  fp32, no contraction, in the order written;
 * a / b is the correctly rounded IEEE division and sqrtf the correctly rounded root; denormals are
 * kept; non-finite radiance is not special.  The GPU, the CPU backend and the tests' numpy statement
 * form the same bits.
 *   mark      per pixel a colour mc[p] and a count mn[p] (unsigned; 0: no mark), one 16-byte record,
 *             allocated on first use.  bdpt_noise_mark sets mc = colors, mn = counter for every
 *             pixel, as they stand after whatever is queued; bdpt_noise_clear sets every mn to 0.
 *             Every call that rewrites the accumulation other than path passes clears the mark too:
 *             bdpt_reset_accum, bdpt_set_scene, bdpt_set_camera, bdpt_write_radiance (and with it
 *             bdpt_load_checkpoint).  Clearing is a flag; it costs nothing while no mark was ever
 *             stored.  The mark is not part of a checkpoint.
 *   pixel p   A = mc[p], B = colors[p], mn = mn[p], cnt = counter[p].  Valid iff mn > 0, cnt > mn and
 *             2*(cnt - mn) >= mn as integers (the fresh samples are at least half the marked ones).
 *               a = (float)mn;  n = (float)cnt;  d = B - A
 *               e1 = (|d.x| + |d.y|) + |d.z|;  s = a / (n - a);  f = sqrtf(s)
 *               lum = (B.x + B.y) + B.z;  den = sqrtf(fmaxf(lum, dark));  e = (e1 * f) / den
 *             (Dammertz et al.'s per-pixel term; sqrt(a/(n-a)) scales |B-A| to the standard error of
 *             B, and is 1 for n = 2a.)  An invalid pixel contributes +0 to sums and reads -1.0f in
 *             the per-pixel plane.
 *   re-mark   (remark != 0) after its estimate is formed from the old mark, a pixel with
 *             0 < cnt < 30000 and cnt >= 2*mn (mn == 0 included) takes the mark: mc = B, mn = cnt.
 *   tile      BDPT_NOISE_TW x BDPT_NOISE_TH (the path kernel's workgroup tile) anchored at (0, 0);
 *             tiles_x = ceil(W/32), tiles_y = ceil(H/8).  Slot k = (y % 8)*32 + (x % 32); slots
 *             outside the frame are invalid.  v[k] = e or +0; eight rounds of v = v[0::2] + v[1::2]
 *             (adjacent pairs) leave S_t; c_t = the number of valid slots;
 *             E_t = c_t ? S_t / (float)c_t : +0.
 *   summary   on the host, from the tile arrays in row-major order: valid_pixels = sum c_t;
 *             valid_tiles = tiles with c_t > 0; mean = (sum (double)S_t) / valid_pixels (a double; 0
 *             when there is none); max_tile: m = 0, if (E_t > m) m = E_t; tiles_over = tiles with
 *             E_t > threshold; pending_pixels = pixels with 0 < cnt < 30000 that are not valid.
 * bdpt_noise_estimate: error_out W*H (or NULL), tile_error and tile_valid tiles_x*tiles_y each (or
 * NULL), summary (or NULL); not all four NULL.  An estimate without any mark is valid: it reports
 * no valid pixel, and with remark it takes the first mark.  bdpt_noise_read_mark /
 * bdpt_noise_write_mark: the mark's colours and counts (either may be NULL on read), for tests and
 * resuming.  bdpt_last_noise_ms: device time of the last estimate's kernel alone (HIP events; wall
 * time on the CPU backend).  All calls are synchronous, ordered after whatever the context has
 * queued, and write nothing but the mark and their own buffers: accumulation, counters, pixels,
 * tables, VLPs, path timing, the auto stream mode's measurements, shards and the reprojection
 * history are untouched.
 * BDPT_EINVAL: NULL parameters, dark not > 0 (NaN rejected), threshold negative or NaN, all outputs
 * NULL, a multi-device context.  BDPT_ESTATE: bdpt_noise_read_mark while no mark was ever stored;
 * bdpt_last_noise_ms before the first estimate.  Defaults: dark 0.01, threshold 0.05, remark 0.
 * bdpt_noise_tile_pending: the last bdpt_noise_estimate's pending count per tile (tiles_x * tiles_y,
 * row-major; their sum is the summary's pending_pixels), so that a caller can tell which tiles are
 * settled (bdpt_path_passes_tiles).  BDPT_ESTATE before the first estimate, BDPT_EINVAL for NULL or a
 * multi-device context. */
#define BDPT_NOISE_TW 32
#define BDPT_NOISE_TH 8
typedef struct { float dark; float threshold; int remark; } bdpt_noise_params;
typedef struct { long long valid_pixels, pending_pixels; int tiles_x, tiles_y, valid_tiles, tiles_over;
                 double mean; float max_tile; } bdpt_noise_summary;
int  bdpt_noise_mark(bdpt_ctx *ctx);
int  bdpt_noise_clear(bdpt_ctx *ctx);
int  bdpt_noise_tiles(const bdpt_ctx *ctx, int *tiles_x, int *tiles_y);
int  bdpt_noise_read_mark(bdpt_ctx *ctx, bdpt_vec *colors, unsigned *counter);
int  bdpt_noise_write_mark(bdpt_ctx *ctx, const bdpt_vec *colors, const unsigned *counter);
int  bdpt_noise_estimate(bdpt_ctx *ctx, const bdpt_noise_params *params, float *error_out,
                         float *tile_error, unsigned *tile_valid, bdpt_noise_summary *summary);
int  bdpt_noise_tile_pending(bdpt_ctx *ctx, unsigned *tile_pending);
int  bdpt_last_noise_ms(bdpt_ctx *ctx, float *ms);

/* ---- noise-guided denoiser: bdpt_denoise with a colour stop that follows the measured variance
 * (no reference counterpart) ----
 * bdpt_denoise stops at colour edges with one absolute constant, which suits a frame of a few passes
 * and over-blurs a converged one.  Here the stop of every pair of pixels is scaled by the variance
 * of their running means, estimated from the noise estimate's mark: with A the mean of the mn marked
 * samples and B the mean of all cnt, |B - A|^2 * mn / (cnt - mn) estimates Var(B) without bias.
 * Guides, eligibility, h, levels and steps are bdpt_denoise's.  fp32, no contraction, in the order
 * written; dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z; 1/x is the correctly rounded reciprocal and
 * a / b the correctly rounded IEEE division; denormals are kept; a tap that is not used is skipped,
 * not weighted by zero; non-finite radiance is not special.  The GPU, the CPU backend and the tests'
 * numpy statement form the same bits.  A variance v "is none" iff v < 0 (stored as -1.0f; an
 * estimate is >= +0 or NaN); has(v) = !(v < 0).
 *   raw       per pixel p: B = colors[p], cnt = counter[p] as they stand, A = mc[p], mn = mn[p] (the
 *             mark of bdpt_noise_estimate; a context without a stored mark, or with a cleared one,
 *             has mn = 0 everywhere).  p has an estimate iff mn > 0, cnt > mn and 2*(cnt - mn) >= mn
 *             in 64-bit integers (bdpt_noise_estimate's rule):
 *               a = (float)mn;  n = (float)cnt;  d = B - A;  e2 = dot(d, d)
 *               v0[p] = e2 * (a / (n - a))
 *             otherwise v0[p] = -1.
 *   prefilter one statistic per pixel is too noisy to use alone.  An ineligible p keeps v[p] = v0[p].
 *             For an eligible centre p: sv = sh = +0; for j = 0..4 (dy = j-2), for i = 0..4
 *             (dx = i-2), a tap q inside the frame with id[q] == id[p] and has(v0[q]) adds
 *               sv = sv + (h[j]*h[i]) * v0[q];  sh = sh + h[j]*h[i]
 *             and v[p] = sv / sh; no tap counted: v[p] = -1.
 *   level k   = 0 .. levels-1, step s = 2^k, isc_k as for bdpt_denoise, s2 = noise_sigma*noise_sigma,
 *             eps = BDPT_DENOISE_NOISE_EPS.  An ineligible pixel is copied through, colour and
 *             variance.  For an eligible centre p: sw = sv = +0, sc = (+0, +0, +0); for j = 0..4
 *             (rows, outer), for i = 0..4, a tap q inside the frame with id[q] == id[p] adds
 *               d  = dot(n_p, n_q);  wn = max(d, 0), then wn = wn*wn normal_power times
 *               dc = cur[q] - cur[p];  e2 = dot(dc, dc)
 *               has(v[p]) and has(v[q]):  t = s2 * (v[p] + v[q]) + eps;  wc = t * (1 / (t + e2))
 *               otherwise:                wc = 1 / (1 + e2*isc_k)          (bdpt_denoise's stop)
 *               w  = ((h[j]*h[i]) * wn) * wc
 *               sw = sw + w;  sc = sc + w*cur[q]
 *               has(v[p]):  sv = sv + (w*w) * (has(v[q]) ? v[q] : v[p])
 *             and r = 1/sw, out = sc * r; the centre's new variance is (sv * r) * r where has(v[p]),
 *             and stays -1 where not.  Level k+1 reads level k's colours and variances.
 * Why: two means of one true colour differ by a variance of v[p] + v[q], so a colour distance is an
 * edge in proportion to it; there is no 4^k factor on that branch because the carried variance
 * itself shrinks as the filter averages (sum w^2 v / (sum w)^2 is the variance of the weighted mean of
 * independent taps).  Consequence: while no pixel has an estimate -- no mark stored, a cleared mark,
 * a mark that is valid nowhere -- every tap takes the second branch and the call returns
 * bdpt_denoise's bits for the same levels, normal_power, sigma_color and materials.
 *   levels 1..8, normal_power 0..6, sigma_color > 0 (+inf allowed), noise_sigma > 0 and finite.
 *   Defaults: levels 4, normal_power 5, sigma_color 0.5, noise_sigma 1, materials DIFFUSE.
 * colors_out, rgba_out: as bdpt_denoise's, either may be NULL, not both.  variance_out (or NULL):
 * W*H floats, the carried variance after the last level, -1 where there is none.  Synchronous,
 * ordered after whatever is queued; it only reads the accumulation, the counters and the mark and
 * writes nothing but its own buffers.  BDPT_EINVAL: NULL or out-of-range parameters, colors_out and
 * rgba_out both NULL, a multi-device context.  BDPT_ESTATE: no camera set.
 * bdpt_last_denoise_noise_ms: device time of the last successful call's kernels alone (HIP events;
 * wall time on the CPU backend), BDPT_ESTATE before the first. */
#define BDPT_DENOISE_NOISE_EPS 1e-12f
typedef struct { int levels; int normal_power; float sigma_color; int materials;
                 float noise_sigma; } bdpt_denoise_noise_params;
int  bdpt_denoise_noise(bdpt_ctx *ctx, const bdpt_denoise_noise_params *params, bdpt_vec *colors_out,
                        unsigned char *rgba_out, float *variance_out);
int  bdpt_last_denoise_noise_ms(bdpt_ctx *ctx, float *ms);

/* ---- optional display: HIP-GL interop ----
 * The caller owns the window, its OpenGL context (current on the calling thread) and a
 * pixel-unpack buffer of at least 4*W*H bytes (glGenBuffers + glBufferData(GL_PIXEL_UNPACK_BUFFER,
 * 4*W*H, NULL, GL_DYNAMIC_COPY), as CreatePBO smallpt_cpu.c:112-123 makes it).
 * bdpt_gl_register_pbo replaces cudaGLRegisterBufferObject (smallpt_cpu.c:122): BDPT_EINVAL when
 * no GL context is current (GLX or EGL, looked up in the libraries the process has loaded) or on
 * the CPU backend.  bdpt_gl_publish replaces IdleFunc's map / UpdateRendering / unmap bracket
 * (display_func.c:199-215): it maps the buffer, copies the frame's 8-bit pixels into it (the
 * layout of bdpt_read_pixels: RGBA, bottom row first, as glTexSubImage2D takes it; for a
 * multi-device context the assembled frame), unmaps it -- on every path -- and synchronises;
 * BDPT_ESTATE before a register, BDPT_EINVAL when the buffer is smaller than the frame.
 * bdpt_gl_unregister (also done by bdpt_destroy) must run while the GL context still exists. */
int  bdpt_gl_register_pbo(bdpt_ctx *ctx, unsigned int pbo);
int  bdpt_gl_publish(bdpt_ctx *ctx);
int  bdpt_gl_unregister(bdpt_ctx *ctx);

/* ---- checkpoint / resume of the accumulation (no reference counterpart: the reference keeps
 * it only in dev_colors/dev_counter) ---- */
/* Upload colors/counter (W*H each; the counterpart of bdpt_read_radiance); pixels are
 * recomputed.  Rendering then continues from that state bit for bit. */
int  bdpt_write_radiance(bdpt_ctx *ctx, const bdpt_vec *colors, const unsigned *counter);
/* File = header {"BDPTCKP2", W, H, host_bytes, n_spheres, table seed, flags} + camera + spheres +
 * the 4096 VLPs + colors + counter + host_bytes of caller state (e.g. its bdpt_pass_state and
 * current_sample, so the pass schedule resumes too).  The render state travels with the frame: a
 * run whose camera or scene was edited (KeyFunc -> ReInit / ReInitScene) resumes with the edited
 * camera, scene, MT table and VLPs, not the scene file's.  Written to a temporary file, flushed to
 * disk (fsync) and renamed into place.  Load checks W, H and host_bytes against the context, then
 * restores scene, camera, table, VLPs and accumulation (the caller re-reads its own copies with
 * bdpt_get_camera / bdpt_get_scene).  The scene upload is skipped when the context already holds
 * the same spheres byte for byte.  If a restore step fails, the context's previous scene, camera,
 * table, VLPs and accumulation are put back (best effort) and the step's error is returned; a
 * version-1 file ("BDPTCKP1", round 2) is refused with a message that says so. */
int  bdpt_save_checkpoint(bdpt_ctx *ctx, const char *path, const void *host_state, unsigned host_bytes);
int  bdpt_load_checkpoint(bdpt_ctx *ctx, const char *path, void *host_state, unsigned host_bytes);

/* ---- host utilities kept for the drop-in (display_func.c / smallpt_cpu.c) ---- */

/* ReadScene display_func.c:112-175. *spheres is malloc'd; free with bdpt_free_scene. */
int  bdpt_read_scene(const char *path, bdpt_camera *camera, bdpt_sphere **spheres,
                     unsigned *n_spheres);
void bdpt_free_scene(bdpt_sphere *spheres);
/* The built-in CornellSpheres scene (scene.h:7-18) and camera (smallpt_cpu.c:404-405),
 * used when the host is started without arguments. Returns the sphere count (9). */
unsigned bdpt_default_scene(bdpt_camera *camera, bdpt_sphere *spheres_out /* >= 9 */);
/* UpdateCamera display_func.c:177-190 (width/height are the internal sizes). */
void bdpt_update_camera(bdpt_camera *camera, int width, int height);
/* Camera moves of KeyFunc / SpecialFunc (display_func.c:278-437), headless.
 * key: 'a','d','w','s','r','f' or BDPT_KEY_*; returns 1 if the camera moved (caller then
 * does ReInit), 0 for keys that do not move the camera. */
#define BDPT_KEY_UP        0x101
#define BDPT_KEY_DOWN      0x102
#define BDPT_KEY_LEFT      0x103
#define BDPT_KEY_RIGHT     0x104
#define BDPT_KEY_PAGE_UP   0x105
#define BDPT_KEY_PAGE_DOWN 0x106
int  bdpt_camera_key(bdpt_camera *camera, int key);
/* Sphere edits of KeyFunc ('4','6','8','2','9','3': display_func.c:347-370). Returns 1 if moved. */
int  bdpt_sphere_key(bdpt_sphere *spheres, unsigned n_spheres, int current_sphere, int key);
/* SavePPM smallpt_cpu.c:239-262: ASCII P3, rows written bottom-up. */
int  bdpt_save_ppm(const char *path, const unsigned char *rgba, int width, int height);
/* Binary P6 with the same header numbers and bottom-up rows (no reference counterpart). */
int  bdpt_save_ppm_binary(const char *path, const unsigned char *rgba, int width, int height);
/* SavePPM file name smallpt_cpu.c:245, "max1_secondi%.3f_exe%d.ppm", bounded by `size`. */
int  bdpt_ppm_name(char *buf, int size, float total_time, int current_sample);
/* The 256 thresholds behind the kernel's toInt (vec.h:34): thr[k] = smallest float whose
 * toInt is >= k (thr[0] = -inf), with correctly-rounded powf semantics. */
void bdpt_gamma_thresholds(float thr[256]);
/* glibc-compatible rand()/srand() (TYPE_3 additive feedback, 31-word state), so the sid
 * sequence `rand() % RAND_N` (smallpt_cpu.c:270, never srand'd => seed 1) is reproducible
 * independently of the C library in use. */
typedef struct { int state[31]; int f, r; } bdpt_rand_state;
void bdpt_srand(bdpt_rand_state *st, unsigned seed);
int  bdpt_rand(bdpt_rand_state *st);

/* The pass scheduler of the reference: glibc rand() for sid (smallpt_cpu.c:270) and the
 * flag / vlp_index state machine (smallpt_cpu.c:47,292-293,361; display_func.c:44,204-210).
 * Initial state = program start: srand(1), flag = 1, vlp_index = MAX_VLP = 1. */
typedef struct { bdpt_rand_state rng; int flag; int vlp_index; } bdpt_pass_state;
void bdpt_pass_state_init(bdpt_pass_state *ps);
/* UpdateRendering2 epilogue: flag = 2 (smallpt_cpu.c:361). */
void bdpt_pass_state_light(bdpt_pass_state *ps);
/* One UpdateRendering: returns the pass's sid and vlp_index, then applies :292-293.
 * vlp_index is reported modulo LIGHT_POINTS (the reference reads dev_lp out of bounds once it
 * reaches 4096 at ~8191 spp -- survey Appendix A.3; wrapping is the documented fix). */
void bdpt_pass_state_next(bdpt_pass_state *ps, unsigned *sid, int *vlp_index);
/* `npass` consecutive bdpt_pass_state_next calls. */
void bdpt_pass_schedule(bdpt_pass_state *ps, int npass, unsigned *sid, int *vlp_index);

#ifdef __cplusplus
}
#endif
#endif /* BDPT_H */
