// preview_asan.cpp -- TEST INFRASTRUCTURE: the CPU backend's denoised preview
// (bdpt_cpu_preview_denoise, csrc/bdpt_cpu.cpp) under AddressSanitizer + UBSan, driven directly
// with no context layer and no Python (`make asan`, run by tests/test_preview_asan.py):
//   preview_asan <MersenneTwister.dat>
// On a 7x5 and a 40x33 frame of the built-in scene: four passes under the scene's camera, a history
// whose weights hold 0, 1e-30, 0.5, 1, 64, 3e4 and 1e30 in runs, then for a few other cameras one
// pass or a reset accumulation (holes: pixels with no sample at all next to filled ones) and the
// call at levels 0 .. 8 into buffers of exactly the packed size -- at 7x5 every off-centre tap is
// outside the frame from step 8 on, so a read or write outside [H][W] is a report.
// Checked besides: levels = 0 returns bdpt_cpu_reproject's bytes, two calls give the same bytes,
// each output alone equals the joint call, no output is NaN, every carried count is 0 or inside
// [2^-20, 2^40], and the history and the accumulation are only read.  Exit status 0 = clean.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../gpu_bidirectional_raytracer_amd/csrc/bdpt_cpu.h"

static void passes(bdpt_cpu_ctx* c, bdpt_pass_state* ps, int npass) {
    std::vector<unsigned> sid(npass);
    std::vector<int> vlp(npass);
    bdpt_pass_schedule(ps, npass, sid.data(), vlp.data());
    bdpt_cpu_path_passes(c, sid.data(), vlp.data(), npass);
}

static int run(const uint32_t* params, int W, int H) {
    bdpt_camera cam0;
    bdpt_sphere spheres[9];
    const unsigned n = bdpt_default_scene(&cam0, spheres);
    bdpt_update_camera(&cam0, W, H);
    bdpt_cpu_ctx* c = bdpt_cpu_create(spheres, n, W, H, params);
    if (!c) return 1;
    bdpt_cpu_set_camera(c, &cam0);
    bdpt_cpu_light_pass(c, 0);
    bdpt_pass_state ps;
    bdpt_pass_state_init(&ps);
    bdpt_pass_state_light(&ps);
    passes(c, &ps, 4);
    const size_t np = (size_t)W * H;
    int bad = 0, holes = 0, filled_holes = 0, calls = 0;

    std::vector<bdpt_vec> hist_col(np);
    std::vector<float> hist_w(np);
    bdpt_cpu_read_radiance(c, hist_col.data(), nullptr);
    const float weights[7] = {0.f, 1e-30f, 0.5f, 1.f, 64.f, 3e4f, 1e30f};
    for (size_t i = 0; i < np; i++) hist_w[i] = weights[(i / 3) % 7];
    bdpt_cpu_history_write(c, &cam0, hist_col.data(), hist_w.data());

    std::vector<bdpt_camera> cams;
    cams.push_back(cam0);
    bdpt_camera k = cam0;
    bdpt_camera_key(&k, BDPT_KEY_LEFT);
    bdpt_update_camera(&k, W, H);
    cams.push_back(k);
    k = cam0;
    bdpt_camera_key(&k, 'a');
    bdpt_update_camera(&k, W, H);
    cams.push_back(k);

    for (size_t ci = 0; ci < cams.size(); ci++)
        for (int one_pass = 0; one_pass < 2; one_pass++) {
            bdpt_cpu_set_camera(c, &cams[ci]);
            bdpt_cpu_reset_accum(c);
            if (one_pass) passes(c, &ps, 1);
            std::vector<bdpt_vec> in(np);
            bdpt_cpu_read_radiance(c, in.data(), nullptr);
            for (int levels = 0; levels <= 8; levels++) {
                bdpt_preview_params p;
                p.rp.materials = levels % 2 ? BDPT_DENOISE_ALL : BDPT_DENOISE_DIFFUSE;
                p.rp.max_history = levels % 3 ? 64.f : INFINITY;
                p.rp.plane_tol = 0.01f;
                p.levels = levels;
                p.normal_power = levels % 7;
                p.sigma_color = levels == 4 ? INFINITY : 0.5f;
                p.count_ref = levels % 2 ? 8.f : 100.f;
                std::vector<bdpt_vec> a(np), b(np), only_col(np);
                std::vector<float> wa(np), wb(np), only_w(np);
                std::vector<unsigned char> pa(4 * np), pb(4 * np), only_px(4 * np);
                bdpt_cpu_preview_denoise(c, &p, a.data(), wa.data(), pa.data());
                bdpt_cpu_preview_denoise(c, &p, b.data(), wb.data(), pb.data());
                bdpt_cpu_preview_denoise(c, &p, only_col.data(), nullptr, nullptr);
                bdpt_cpu_preview_denoise(c, &p, nullptr, only_w.data(), nullptr);
                bdpt_cpu_preview_denoise(c, &p, nullptr, nullptr, only_px.data());
                calls += 5;
                bad += memcmp(a.data(), b.data(), sizeof(bdpt_vec) * np) != 0 || pa != pb ||
                       memcmp(wa.data(), wb.data(), sizeof(float) * np) != 0;
                bad += memcmp(a.data(), only_col.data(), sizeof(bdpt_vec) * np) != 0 || pa != only_px ||
                       memcmp(wa.data(), only_w.data(), sizeof(float) * np) != 0;
                std::vector<bdpt_vec> r(np);
                std::vector<float> wr(np);
                std::vector<unsigned char> pr(4 * np);
                bdpt_cpu_reproject(c, &p.rp, r.data(), wr.data(), pr.data());
                if (levels == 0) {
                    bad += memcmp(a.data(), r.data(), sizeof(bdpt_vec) * np) != 0 || pa != pr ||
                           memcmp(wa.data(), wr.data(), sizeof(float) * np) != 0;
                    continue;
                }
                for (size_t i = 0; i < np; i++) {
                    bad += a[i].x != a[i].x || a[i].y != a[i].y || a[i].z != a[i].z;
                    bad += !(wa[i] == 0.f || (wa[i] >= 0x1p-20f && wa[i] <= 0x1p40f));
                    if (wr[i] == 0.f) {
                        holes++;
                        filled_holes += wa[i] > 0.f;
                    }
                }
            }
            std::vector<bdpt_vec> after(np), hc(np);
            std::vector<float> hm(np);
            bdpt_cpu_read_radiance(c, after.data(), nullptr);
            bdpt_cpu_history_read(c, hc.data(), hm.data());
            bad += memcmp(after.data(), in.data(), sizeof(bdpt_vec) * np) != 0;      // only read
            bad += memcmp(hc.data(), hist_col.data(), sizeof(bdpt_vec) * np) != 0 ||
                   memcmp(hm.data(), hist_w.data(), sizeof(float) * np) != 0;
        }
    printf("%dx%d: calls %d, holes %d, holes filled %d, mismatches %d\n", W, H, calls, holes, filled_holes, bad);
    bad += !(holes && filled_holes);
    bdpt_cpu_destroy(c);
    return bad;
}

int main(int argc, char** argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: preview_asan <MersenneTwister.dat>\n");
        return 2;
    }
    static uint32_t params[4 * BDPT_MT_RNG_COUNT];
    FILE* f = fopen(argv[1], "rb");
    if (!f || fread(params, sizeof params, 1, f) != 1) {
        fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    fclose(f);
    const int bad = run(params, 7, 5) + run(params, 40, 33);
    return bad ? 1 : 0;
}
