// tiles_asan.cpp -- TEST INFRASTRUCTURE: the CPU backend's path passes over a tile mask
// (bdpt_cpu_path_passes with tile_mask, csrc/bdpt_cpu.cpp) under AddressSanitizer + UBSan, driven
// directly with no context layer and no Python (`make asan`, run by tests/test_tiles_asan.py):
//   tiles_asan <MersenneTwister.dat>
// On a 97x65 frame (4 x 9 tiles, the last column one pixel wide, the last row one pixel high) and a
// 33x9 frame (2 x 2 tiles, three of them partial) of the built-in scene, with masks in heap buffers
// of exactly tiles_x * tiles_y bytes, so that a tile read outside the mask is a report: a checkerboard
// with the corner tile (A), the last column and row plus one interior tile (B) and the empty mask
// (Z), four passes each after four unmasked ones.  Checked besides: a pixel of a masked-in tile holds
// what an unmasked context holds after the same passes, every other pixel keeps colours, counter and
// pixel bytes, and the empty mask changes nothing.  Exit status 0 = clean.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../gpu_bidirectional_raytracer_amd/csrc/bdpt_cpu.h"

struct Frame {
    std::vector<bdpt_vec> col;
    std::vector<unsigned> cnt;
    std::vector<unsigned char> px;
};

static Frame read(const bdpt_cpu_ctx* c, size_t np) {
    Frame f{std::vector<bdpt_vec>(np), std::vector<unsigned>(np), std::vector<unsigned char>(4 * np)};
    bdpt_cpu_read_radiance(c, f.col.data(), f.cnt.data());
    bdpt_cpu_read_pixels(c, f.px.data());
    return f;
}

static bool same_pixel(const Frame& a, const Frame& b, size_t i) {
    return memcmp(&a.col[i], &b.col[i], sizeof(bdpt_vec)) == 0 && a.cnt[i] == b.cnt[i] &&
           memcmp(&a.px[4 * i], &b.px[4 * i], 4) == 0;
}

static bdpt_cpu_ctx* make(const uint32_t* params, int W, int H) {
    bdpt_camera cam;
    bdpt_sphere spheres[9];
    const unsigned n = bdpt_default_scene(&cam, spheres);
    bdpt_update_camera(&cam, W, H);
    bdpt_cpu_ctx* c = bdpt_cpu_create(spheres, n, W, H, params);
    if (!c) return nullptr;
    bdpt_cpu_set_camera(c, &cam);
    bdpt_cpu_light_pass(c, 0);
    return c;
}

static int run(const uint32_t* params, int W, int H) {
    const int tx = (W + BDPT_NOISE_TW - 1) / BDPT_NOISE_TW, ty = (H + BDPT_NOISE_TH - 1) / BDPT_NOISE_TH;
    const size_t np = (size_t)W * H, nt = (size_t)tx * ty;
    bdpt_cpu_ctx *c = make(params, W, H), *u = make(params, W, H);   // masked and unmasked
    if (!c || !u) return 1;
    bdpt_pass_state ps;
    bdpt_pass_state_init(&ps);
    bdpt_pass_state_light(&ps);
    unsigned sid[16];
    int vlp[16];
    bdpt_pass_schedule(&ps, 16, sid, vlp);
    bdpt_cpu_path_passes(c, sid, vlp, 4);
    bdpt_cpu_path_passes(u, sid, vlp, 4, nullptr);
    int bad = 0, p = 4;
    long long rendered = 0, kept = 0;
    for (const char name : {'A', 'B', 'Z'}) {
        std::vector<unsigned char> mask(nt);                         // exactly the mask's size, on the heap
        for (int t = 0; t < (int)nt; t++) {
            const int x = t % tx, y = t / tx;
            mask[t] = name == 'A' ? (x + y) % 2 == (tx + ty) % 2
                    : name == 'B' ? (x == tx - 1 || y == ty - 1 || (x == (tx > 1) && y == ty / 2)) * 7 : 0;
        }
        const Frame before = read(c, np);
        bdpt_cpu_path_passes(c, sid + p, vlp + p, 4, mask.data());
        // the unmasked context renders the same passes from the masked context's state
        bdpt_cpu_write_radiance(u, before.col.data(), before.cnt.data());
        bdpt_cpu_path_passes(u, sid + p, vlp + p, 4);
        const Frame after = read(c, np), full = read(u, np);
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) {
                const size_t i = (size_t)y * W + x;
                const bool in = mask[(size_t)(y / BDPT_NOISE_TH) * tx + x / BDPT_NOISE_TW] != 0;
                // (write_radiance recomputes the pixel bytes from the colours: they agree with the
                // masked context's, whose bytes came from the same colours)
                bad += !same_pixel(after, in ? full : before, i);
                rendered += in;
                kept += !in;
                if (in) bad += after.cnt[i] != before.cnt[i] + 4;
            }
        p += 4;
    }
    printf("%dx%d: tiles %dx%d, pixel-calls rendered %lld kept %lld, mismatches %d\n", W, H, tx, ty, rendered, kept, bad);
    bdpt_cpu_destroy(c);
    bdpt_cpu_destroy(u);
    return bad != 0;
}

int main(int argc, char** argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: tiles_asan <MersenneTwister.dat>\n");
        return 2;
    }
    static uint32_t params[4 * BDPT_MT_RNG_COUNT];
    FILE* f = fopen(argv[1], "rb");
    if (!f || fread(params, sizeof params, 1, f) != 1) {
        fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    fclose(f);
    int bad = run(params, 97, 65);
    bad += run(params, 33, 9);
    return bad ? 1 : 0;
}
