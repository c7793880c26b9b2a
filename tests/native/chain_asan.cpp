// chain_asan.cpp -- TEST INFRASTRUCTURE: the CPU backend's chain buffers and the denoiser guided
// through them (bdpt_cpu_render_chain, bdpt_cpu_denoise with BDPT_DENOISE_THROUGH; csrc/bdpt_cpu.cpp)
// under AddressSanitizer + UBSan, driven directly with no context layer and no Python (`make asan`,
// run by tests/test_chain_asan.py):
//   chain_asan <MersenneTwister.dat> <cornell_mirror.scn>
// On a 33x9 frame: create, set the camera, generate the table, then the whole frame and a window,
// TRANSMIT without jitter and PASS with it, into buffers of exactly the packed size -- a write past
// [h][w] is a report -- a two-plane request, and the denoiser with materials = through after four
// passes.  The window must equal the frame's slice.  Exit status 0 = clean.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../gpu_bidirectional_raytracer_amd/csrc/bdpt_cpu.h"

struct Planes {
    std::vector<int> id, first_id, kind, bounces;
    std::vector<float> t, dp;
    std::vector<bdpt_vec> position, normal, dir, throughput;
    bdpt_chain_buffers out;
    explicit Planes(size_t n)
        : id(n), first_id(n), kind(n), bounces(n), t(n), dp(n), position(n), normal(n), dir(n), throughput(n) {
        out.id = id.data(); out.first_id = first_id.data(); out.kind = kind.data(); out.bounces = bounces.data();
        out.t = t.data(); out.dp = dp.data(); out.position = position.data(); out.normal = normal.data();
        out.dir = dir.data(); out.throughput = throughput.data();
    }
};

int main(int argc, char** argv) {
    if (argc < 3) {
        fprintf(stderr, "usage: chain_asan <MersenneTwister.dat> <scene.scn>\n");
        return 2;
    }
    static uint32_t params[4 * BDPT_MT_RNG_COUNT];
    FILE* f = fopen(argv[1], "rb");
    if (!f || fread(params, sizeof params, 1, f) != 1) {
        fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    fclose(f);
    const int W = 33, H = 9;
    bdpt_camera cam;
    bdpt_sphere* spheres = nullptr;
    unsigned n = 0;
    if (bdpt_read_scene(argv[2], &cam, &spheres, &n) != BDPT_OK) {
        fprintf(stderr, "cannot read %s\n", argv[2]);
        return 2;
    }
    bdpt_update_camera(&cam, W, H);
    bdpt_cpu_ctx* c = bdpt_cpu_create(spheres, n, W, H, params);
    if (!c) return 2;
    bdpt_cpu_set_camera(c, &cam);
    bdpt_cpu_generate_rand(c, 15);

    int bad = 0;
    const int branches[2] = {BDPT_CHAIN_TRANSMIT, BDPT_CHAIN_PASS};
    for (int jitter = 0; jitter < 2; jitter++) {
        Planes whole((size_t)W * H);
        bdpt_cpu_render_chain(c, 0, 0, W, H, jitter, 7u, branches[jitter], &whole.out);
        const int x0 = 7, y0 = 3, w = 13, h = 5;
        Planes win((size_t)w * h);
        bdpt_cpu_render_chain(c, x0, y0, w, h, jitter, 7u, branches[jitter], &win.out);
        int through = 0;
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) {
                const size_t k = (size_t)y * w + x, i = (size_t)(y0 + y) * W + (x0 + x);
                through += win.bounces[k] > 0;
                bad += win.id[k] != whole.id[i] || win.first_id[k] != whole.first_id[i] || win.kind[k] != whole.kind[i] ||
                       win.bounces[k] != whole.bounces[i] || memcmp(&win.t[k], &whole.t[i], 4) != 0 ||
                       memcmp(&win.dp[k], &whole.dp[i], 4) != 0 ||
                       memcmp(&win.position[k], &whole.position[i], 12) != 0 ||
                       memcmp(&win.normal[k], &whole.normal[i], 12) != 0 ||
                       memcmp(&win.dir[k], &whole.dir[i], 12) != 0 ||
                       memcmp(&win.throughput[k], &whole.throughput[i], 12) != 0;
            }
        // a partial request: kind and throughput of the last pixel, the other pointers NULL
        bdpt_chain_buffers two;
        memset(&two, 0, sizeof two);
        std::vector<int> kind(1);
        std::vector<bdpt_vec> thr(1);
        two.kind = kind.data();
        two.throughput = thr.data();
        bdpt_cpu_render_chain(c, W - 1, H - 1, 1, 1, jitter, 7u, branches[jitter], &two);
        bad += kind[0] != whole.kind[(size_t)W * H - 1] || memcmp(&thr[0], &whole.throughput[(size_t)W * H - 1], 12) != 0;
        printf("jitter %d: window pixels through a mirror or glass %d of %d, mismatches so far %d\n", jitter, through,
               w * h, bad);
    }

    // four passes, then the denoiser guided through the chain, into buffers of exactly the frame's size
    bdpt_cpu_light_pass(c, 0);
    const unsigned sid[4] = {7u, 1234u, 99999u, BDPT_RAND_N - 1u};
    const int vlp[4] = {1, 2, 3, 4};
    bdpt_cpu_path_passes(c, sid, vlp, 4);
    const bdpt_denoise_params p = {4, 5, 0.5f, BDPT_DENOISE_THROUGH};
    std::vector<bdpt_vec> col((size_t)W * H), raw((size_t)W * H);
    std::vector<unsigned char> rgba(4 * (size_t)W * H);
    bdpt_cpu_denoise(c, &p, col.data(), rgba.data());
    bdpt_cpu_read_radiance(c, raw.data(), nullptr);
    int changed = 0;
    for (size_t i = 0; i < col.size(); i++) changed += memcmp(&col[i], &raw[i], 12) != 0;
    printf("denoise through: %d of %d pixels filtered\n", changed, W * H);
    bad += changed == 0;
    bdpt_cpu_destroy(c);
    bdpt_free_scene(spheres);
    return bad ? 1 : 0;
}
