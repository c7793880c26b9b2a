// denoise_asan.cpp -- TEST INFRASTRUCTURE: the CPU backend's denoiser (bdpt_cpu_denoise,
// csrc/bdpt_cpu.cpp) under AddressSanitizer + UBSan, driven directly with no context layer and no
// Python (`make asan`, run by tests/test_denoise_asan.py):
//   denoise_asan <MersenneTwister.dat>
// On a 7x5 and a 33x9 frame of the built-in scene: create, set the camera, a light pass and four
// path passes, then the denoiser with 1, 3 and 8 levels (steps up to 128: every off-centre tap of
// the later levels is outside the frame), both material modes, into buffers of exactly the packed
// size -- a read or write outside [H][W] is a report.  Checked besides: two calls give the same
// bytes, pixels that show no DIFF sphere keep the input's bits, and a colours-only and a
// pixels-only request equal the joint one.  Exit status 0 = clean.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../gpu_bidirectional_raytracer_amd/csrc/bdpt_cpu.h"

static int run(const uint32_t* params, int W, int H) {
    bdpt_camera cam;
    bdpt_sphere spheres[9];
    const unsigned n = bdpt_default_scene(&cam, spheres);
    bdpt_update_camera(&cam, W, H);
    bdpt_cpu_ctx* c = bdpt_cpu_create(spheres, n, W, H, params);
    if (!c) return 1;
    bdpt_cpu_set_camera(c, &cam);
    bdpt_cpu_light_pass(c, 0);
    bdpt_pass_state ps;
    bdpt_pass_state_init(&ps);
    bdpt_pass_state_light(&ps);
    unsigned sid[4];
    int vlp[4];
    bdpt_pass_schedule(&ps, 4, sid, vlp);
    bdpt_cpu_path_passes(c, sid, vlp, 4);

    const size_t np = (size_t)W * H;
    std::vector<bdpt_vec> in(np);
    bdpt_cpu_read_radiance(c, in.data(), nullptr);
    std::vector<int> id(np);
    bdpt_aov_buffers g;
    memset(&g, 0, sizeof g);
    g.id = id.data();
    bdpt_cpu_render_aov(c, 0, 0, W, H, 0, 0u, &g);

    int bad = 0, filtered = 0;
    const int levels[3] = {1, 3, 8};
    for (int materials = 0; materials < 2; materials++)
        for (int l = 0; l < 3; l++) {
            const bdpt_denoise_params p = {levels[l], l == 1 ? 0 : 5, l == 2 ? 1e-3f : 0.5f, materials};
            std::vector<bdpt_vec> a(np), b(np), only_col(np);
            std::vector<unsigned char> pa(4 * np), pb(4 * np), only_px(4 * np);
            bdpt_cpu_denoise(c, &p, a.data(), pa.data());
            bdpt_cpu_denoise(c, &p, b.data(), pb.data());
            bdpt_cpu_denoise(c, &p, only_col.data(), nullptr);
            bdpt_cpu_denoise(c, &p, nullptr, only_px.data());
            bad += memcmp(a.data(), b.data(), sizeof(bdpt_vec) * np) != 0 || pa != pb;
            bad += memcmp(a.data(), only_col.data(), sizeof(bdpt_vec) * np) != 0 || pa != only_px;
            for (size_t i = 0; i < np; i++) {
                const bool eligible = id[i] >= 0 && (materials == BDPT_DENOISE_ALL || spheres[id[i]].refl == BDPT_DIFF);
                if (!eligible) bad += memcmp(&a[i], &in[i], sizeof(bdpt_vec)) != 0;
                else filtered++;
            }
        }
    std::vector<bdpt_vec> after(np);
    bdpt_cpu_read_radiance(c, after.data(), nullptr);
    bad += memcmp(after.data(), in.data(), sizeof(bdpt_vec) * np) != 0;   // the accumulation is only read
    printf("%dx%d: filtered pixels %d, mismatches %d\n", W, H, filtered, bad);
    bdpt_cpu_destroy(c);
    return bad;
}

int main(int argc, char** argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: denoise_asan <MersenneTwister.dat>\n");
        return 2;
    }
    static uint32_t params[4 * BDPT_MT_RNG_COUNT];
    FILE* f = fopen(argv[1], "rb");
    if (!f || fread(params, sizeof params, 1, f) != 1) {
        fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    fclose(f);
    const int bad = run(params, 7, 5) + run(params, 33, 9);
    return bad ? 1 : 0;
}
