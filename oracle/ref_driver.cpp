/*
 * TEST INFRASTRUCTURE ONLY: the host side of oracle/_ref/libref.so.
 *
 * libref.so is the reference's own src/device.cu and src/MersenneTwister_kernel.cu compiled in
 * place as host C++ behind oracle/ref_shim.h (see the Makefile).  This file replays, one simulated
 * thread after another, the launches of the reference's host program:
 *   - ref_mt607:       loadMTGPU + seedMTGPU + RandomGPU<<<32,128>>>(d_Rand, N_PER_RNG)
 *                      (smallpt_cpu.c:185,321-322);
 *   - ref_light_pass:  per emitter GetRayKernel + RadianceLightTracingKernel over
 *                      <<<RAYNGRID,RAYNTHREAD>>> with sid = 0 (smallpt_cpu.c:311-359);
 *   - ref_path_passes: RadiancePathTracingKernel<<<ceil(W/19) x ceil(H/19), 19x19>>> once per pass
 *                      (smallpt_cpu.c:270-278), with inverse_width = 14./W and
 *                      inverse_height = 10.5/H (smallpt_cpu.c:411-412).
 *
 * Launch range.  Only the threads with x < W and y < H are run.  The kernel's own guard is
 * `x<=width` (device.cu:556) with i = y*width+x (device.cu:557) and no guard on y: the thread
 * x == W of row y computes the same pixel index as the thread x == 0 of row y+1, and the threads
 * with y >= H index past the frame.  Both threads of such a pair read-modify-write colors[i] and
 * counter[i] unsynchronised: a data race in the reference whose outcome depends on the hardware
 * schedule.  The defined part of the launch is x < W, y < H; dev_lp starts zeroed (the reference
 * cudaMallocs it and reads entries no light path wrote).
 */
#include <cstdint>
#include <vector>

#include "vec.h"
#include "geom.h"
#include "camera.h"
#include "cons.h"

thread_local ref_dim3 threadIdx, blockIdx, blockDim;

/* smallpt_cpu.c:30,67-69: AlignUp(DivideRoundUp(7680000, 4096), 2) = 1876 */
static const int MT_RNG_COUNT = 4096;
static const int N_PER_RNG = 1876;
static const int RAND_N = MT_RNG_COUNT * N_PER_RNG;

/* the entry points of the two reference sources (declared as smallpt_cpu.c:73-96 declares them) */
void loadMTGPU(const char *fname);
void seedMTGPU(unsigned int seed);
__global__ void RandomGPU(float *d_Random, int nPerRng);
__global__ void GetRayKernel(const Sphere light, Ray *dev_data, float *d_Rand, int current_sample,
                             int rand_count, unsigned int seed_id);
__global__ void RadianceLightTracingKernel(Sphere *spheres, unsigned int sphereCount, Ray *start_ray,
                                           float *d_Rand, int id_light, int rand_count, Camera camera,
                                           Vec *colors, unsigned int *counter, LightPath *dev_lp,
                                           float inv_width, float inv_height, float width, float height,
                                           unsigned int seed_id);
__global__ void RadiancePathTracingKernel(Sphere *spheres, unsigned int sphereCount, float *d_Rand,
                                          int rand_count, Camera camera, Vec *colors, unsigned int *counter,
                                          uchar4 *pixels, float inv_width, float inv_height, float width,
                                          float height, unsigned int seed_id, unsigned int param,
                                          LightPath *dev_lp, int vlp_index);

static void launch_1d(unsigned grid, unsigned block, unsigned b, unsigned t)
{
    blockDim = {block, 1, 1};
    blockIdx = {b, 0, 0};
    threadIdx = {t, 0, 0};
    (void)grid;
}

extern "C" {

int ref_rand_n(void) { return RAND_N; }
int ref_light_points(void) { return LIGHT_POINTS * DEPTH; }
int ref_platform_libm(void)
{
#ifdef REF_PLATFORM_LIBM
    return 1;
#else
    return 0;
#endif
}

/* 0 on success, -1 when the parameter file cannot be read (loadMTGPU would exit(0)). */
int ref_mt607(const char *dat_path, unsigned seed, float *out /* RAND_N */)
{
    FILE *f = fopen(dat_path, "rb");
    if (!f) return -1;
    fseek(f, 0, SEEK_END);
    const long sz = ftell(f);
    fclose(f);
    if (sz < (long)(MT_RNG_COUNT * 16)) return -1;
    loadMTGPU(dat_path);
    seedMTGPU(seed);
    for (unsigned b = 0; b < 32; b++)
        for (unsigned t = 0; t < 128; t++) {
            launch_1d(32, 128, b, t);
            RandomGPU(out, N_PER_RNG);
        }
    return 0;
}

/* UpdateRendering2's loop body for every emitter; lp (DEPTH*LIGHT_POINTS) is updated in place. */
void ref_light_pass(const Sphere *spheres, unsigned n, const float *rnd, int current_sample,
                    const Camera *cam, int W, int H, LightPath *lp)
{
    std::vector<Sphere> sp(spheres, spheres + n);
    std::vector<Ray> rays(RAYNGRID * RAYNTHREAD);
    float *d_rand = const_cast<float *>(rnd);
    Camera camera;
    memset(&camera, 0, sizeof camera);
    if (cam) camera = *cam;
    const float inv_w = 14. / W, inv_h = 10.5 / H;
    for (unsigned i = 0; i < n; i++) {
        const Sphere *light = &sp[i];
        if (viszero(light->e)) continue;
        const unsigned sid = 0;
        for (unsigned b = 0; b < RAYNGRID; b++)
            for (unsigned t = 0; t < RAYNTHREAD; t++) {
                launch_1d(RAYNGRID, RAYNTHREAD, b, t);
                GetRayKernel(*light, rays.data(), d_rand, current_sample, RAND_N, sid);
            }
        for (unsigned b = 0; b < RAYNGRID; b++)
            for (unsigned t = 0; t < RAYNTHREAD; t++) {
                launch_1d(RAYNGRID, RAYNTHREAD, b, t);
                RadianceLightTracingKernel(sp.data(), n, rays.data(), d_rand, (int)i, RAND_N, camera,
                                           nullptr, nullptr, lp, inv_w, inv_h, (float)W, (float)H, sid);
            }
    }
}

/* npass x UpdateRendering's launch; colors/counter/pixels (W*H) are read-modify-written. */
void ref_path_passes(const Sphere *spheres, unsigned n, const float *rnd, const Camera *cam, int W, int H,
                     const LightPath *lp, const unsigned *sid, const int *vlp, int npass,
                     Vec *colors, unsigned *counter, uchar4 *pixels)
{
    std::vector<Sphere> sp(spheres, spheres + n);
    float *d_rand = const_cast<float *>(rnd);
    LightPath *dev_lp = const_cast<LightPath *>(lp);
    const float inv_w = 14. / W, inv_h = 10.5 / H;
    const unsigned B = 19;
    const unsigned gx = (unsigned)ceil(W / float(B)), gy = (unsigned)ceil(H / float(B));
    for (int p = 0; p < npass; p++)
        for (unsigned by = 0; by < gy; by++)
            for (unsigned bx = 0; bx < gx; bx++)
                for (unsigned ty = 0; ty < B; ty++)
                    for (unsigned tx = 0; tx < B; tx++) {
                        if (bx * B + tx >= (unsigned)W || by * B + ty >= (unsigned)H)
                            continue;                       /* the launch range, see the header */
                        blockDim = {B, B, 1};
                        blockIdx = {bx, by, 0};
                        threadIdx = {tx, ty, 0};
                        RadiancePathTracingKernel(sp.data(), n, d_rand, RAND_N, *cam, colors, counter, pixels,
                                                  inv_w, inv_h, (float)W, (float)H, sid[p], 30000, dev_lp,
                                                  vlp[p]);
                    }
}

}  /* extern "C" */
