// aov_asan.cpp -- TEST INFRASTRUCTURE: the CPU backend's first-hit feature buffers
// (bdpt_cpu_render_aov, csrc/bdpt_cpu.cpp) under AddressSanitizer + UBSan, driven directly with no
// context layer and no Python (`make asan`, run by tests/test_aov_asan.py):
//   aov_asan <MersenneTwister.dat>
// On a 7x5 frame of the built-in scene: create, set the camera, generate the table, then the
// whole frame and a window, jittered and not, into buffers of exactly the packed size -- a write
// past [h][w] is a report.  The window must equal the frame's slice.  Exit status 0 = clean.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../gpu_bidirectional_raytracer_amd/csrc/bdpt_cpu.h"

struct Planes {
    std::vector<int> id;
    std::vector<float> t, dp;
    std::vector<bdpt_vec> position, normal, dir;
    bdpt_aov_buffers out;
    explicit Planes(size_t n) : id(n), t(n), dp(n), position(n), normal(n), dir(n) {
        out.id = id.data(); out.t = t.data(); out.dp = dp.data();
        out.position = position.data(); out.normal = normal.data(); out.dir = dir.data();
    }
};

int main(int argc, char** argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: aov_asan <MersenneTwister.dat>\n");
        return 2;
    }
    static uint32_t params[4 * BDPT_MT_RNG_COUNT];
    FILE* f = fopen(argv[1], "rb");
    if (!f || fread(params, sizeof params, 1, f) != 1) {
        fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    fclose(f);
    const int W = 7, H = 5;
    bdpt_camera cam;
    bdpt_sphere spheres[9];
    const unsigned n = bdpt_default_scene(&cam, spheres);
    bdpt_update_camera(&cam, W, H);
    bdpt_cpu_ctx* c = bdpt_cpu_create(spheres, n, W, H, params);
    if (!c) return 2;
    bdpt_cpu_set_camera(c, &cam);
    bdpt_cpu_generate_rand(c, 15);

    int bad = 0;
    const unsigned sids[2] = {7u, BDPT_RAND_N - 1u};
    for (int jitter = 0; jitter < 2; jitter++) {
        Planes whole((size_t)W * H);
        bdpt_cpu_render_aov(c, 0, 0, W, H, jitter, sids[jitter], &whole.out);
        const int x0 = 2, y0 = 1, w = 4, h = 3;
        Planes win((size_t)w * h);
        bdpt_cpu_render_aov(c, x0, y0, w, h, jitter, sids[jitter], &win.out);
        int hits = 0;
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) {
                const size_t k = (size_t)y * w + x, i = (size_t)(y0 + y) * W + (x0 + x);
                hits += win.id[k] >= 0;
                bad += win.id[k] != whole.id[i] || memcmp(&win.t[k], &whole.t[i], 4) != 0 ||
                       memcmp(&win.dp[k], &whole.dp[i], 4) != 0 ||
                       memcmp(&win.position[k], &whole.position[i], 12) != 0 ||
                       memcmp(&win.normal[k], &whole.normal[i], 12) != 0 ||
                       memcmp(&win.dir[k], &whole.dir[i], 12) != 0;
            }
        // a partial request: only the ids, the other pointers NULL
        bdpt_aov_buffers only_id;
        memset(&only_id, 0, sizeof only_id);
        std::vector<int> ids(1);
        only_id.id = ids.data();
        bdpt_cpu_render_aov(c, W - 1, H - 1, 1, 1, jitter, sids[jitter], &only_id);
        bad += ids[0] != whole.id[(size_t)W * H - 1];
        printf("jitter %d: window hits %d of %d, mismatches so far %d\n", jitter, hits, w * h, bad);
    }
    bdpt_cpu_destroy(c);
    return bad ? 1 : 0;
}
