// reproject_asan.cpp -- TEST INFRASTRUCTURE: the CPU backend's history and reprojection
// (bdpt_cpu_history_* / bdpt_cpu_reproject, csrc/bdpt_cpu.cpp) under AddressSanitizer + UBSan,
// driven directly with no context layer and no Python (`make asan`, run by
// tests/test_reproject_asan.py):
//   reproject_asan <MersenneTwister.dat>
// On a 7x5 and a 40x33 frame of the built-in scene: four passes and a capture under the scene's
// camera, then, for a list of other cameras, one pass, a reprojection into buffers of exactly the
// packed size and a capture -- a read or write outside [H][W] is a report.  The cameras:
//   * sideways and vertical shifts of 0.3 .. 30 scene units in both directions, so that projected
//     points land in the border cells on all four sides (fx in [-1, 0) and [W-1, W), fy likewise),
//     where one or two of the four taps are outside the frame;
//   * the camera turned by 'left' keys past a right angle and one moved forward through the scene:
//     for part of the frame the point lies beside or behind the old camera (cz = 0 or negative).
// The program restates the projection in double precision only to count that these cases occurred.
// Checked besides: two calls give the same bytes, a pixel that took no history (weight == counter)
// keeps the input's bits, each output alone equals the joint call, and the capture stores what the
// reprojection returned.  Exit status 0 = clean.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../gpu_bidirectional_raytracer_amd/csrc/bdpt_cpu.h"

struct Seen {
    int left = 0, right = 0, top = 0, bottom = 0, behind = 0, took = 0;
};

static void unit3(const bdpt_vec& v, double o[3]) {
    const double l = sqrt((double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z);
    o[0] = v.x / l; o[1] = v.y / l; o[2] = v.z / l;
}

// where the current first hits fall in the old camera's frame (double precision: counting only)
static void classify(const bdpt_camera& c0, int W, int H, const std::vector<int>& id, const std::vector<bdpt_vec>& pos,
                     const std::vector<float>& wout, const std::vector<unsigned>& cnt, Seen* s) {
    double ux[3], uy[3], ud[3];
    unit3(c0.x, ux); unit3(c0.y, uy); unit3(c0.dir, ud);
    for (size_t i = 0; i < id.size(); i++) {
        if (id[i] < 0) continue;
        const double v[3] = {pos[i].x - (double)c0.orig.x, pos[i].y - (double)c0.orig.y, pos[i].z - (double)c0.orig.z};
        const double a = v[0] * ux[0] + v[1] * ux[1] + v[2] * ux[2], b = v[0] * uy[0] + v[1] * uy[1] + v[2] * uy[2];
        const double cz = v[0] * ud[0] + v[1] * ud[1] + v[2] * ud[2];
        if (cz <= 0.) {
            s->behind++;
            continue;
        }
        const double fx = (10. * a / cz + 7.) * (W / 14.), fy = (10. * b / cz + 5.25) * (H / 10.5);
        const bool took = wout[i] > (float)cnt[i];
        s->took += took;
        if (!took || fy < -1. || fy >= H || fx < -1. || fx >= W) continue;
        s->left += fx < 0.;
        s->right += fx >= W - 1;
        s->top += fy < 0.;
        s->bottom += fy >= H - 1;
    }
}

static void one_pass(bdpt_cpu_ctx* c, bdpt_pass_state* ps, int npass) {
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
    one_pass(c, &ps, 4);
    const size_t np = (size_t)W * H;
    int bad = 0;

    std::vector<bdpt_camera> cams;
    const float shifts[5] = {0.3f, 1.f, 3.f, 10.f, 30.f};
    for (int axis = 0; axis < 2; axis++)
        for (int sign = -1; sign <= 1; sign += 2)
            for (float d : shifts) {
                bdpt_camera k = cam0;
                (axis ? k.orig.y : k.orig.x) += sign * d;
                (axis ? k.target.y : k.target.x) += sign * d;
                bdpt_update_camera(&k, W, H);
                cams.push_back(k);
            }
    bdpt_camera turned = cam0, forward = cam0;
    for (int k = 0; k < 40; k++) {                        // past a right angle, whatever the key's step
        bdpt_camera_key(&turned, BDPT_KEY_LEFT);
        bdpt_update_camera(&turned, W, H);
        if (k % 8 == 7) cams.push_back(turned);
    }
    for (int k = 0; k < 12; k++) {
        bdpt_camera_key(&forward, 'w');
        bdpt_update_camera(&forward, W, H);
        if (k % 3 == 2) cams.push_back(forward);
    }

    // the first capture, with no history before it: the four-pass frame itself
    Seen seen;
    const bdpt_reproject_params first = {BDPT_DENOISE_ALL, 64.f, 0.01f};
    bad += bdpt_cpu_history_present(c);
    bdpt_cpu_history_capture(c, &first);
    bad += !bdpt_cpu_history_present(c);
    std::vector<bdpt_vec> hist_col(np);
    std::vector<float> hist_w(np);
    bdpt_cpu_history_read(c, hist_col.data(), hist_w.data());
    std::vector<bdpt_vec> frame0(np);
    std::vector<unsigned> count0(np);
    bdpt_cpu_read_radiance(c, frame0.data(), count0.data());
    bad += memcmp(hist_col.data(), frame0.data(), sizeof(bdpt_vec) * np) != 0;   // no history before: the frame itself
    for (size_t i = 0; i < np; i++) {
        bad += hist_w[i] != (float)count0[i];
        if (i % 7 == 3) hist_w[i] = 0.f;                  // some pixels without history
    }

    for (size_t k = 0; k < cams.size(); k++) {
        bdpt_cpu_history_write(c, &cam0, hist_col.data(), hist_w.data());
        bdpt_cpu_set_camera(c, &cams[k]);
        bdpt_cpu_reset_accum(c);
        one_pass(c, &ps, 1);
        std::vector<bdpt_vec> in(np);
        std::vector<unsigned> cnt(np);
        bdpt_cpu_read_radiance(c, in.data(), cnt.data());
        std::vector<int> id(np);
        std::vector<bdpt_vec> pos(np);
        bdpt_aov_buffers g;
        memset(&g, 0, sizeof g);
        g.id = id.data();
        g.position = pos.data();
        bdpt_cpu_render_aov(c, 0, 0, W, H, 0, 0u, &g);
        for (int materials = 0; materials < 2; materials++) {
            const bdpt_reproject_params p = {materials, k % 2 ? 64.f : 1.f, k % 3 ? 0.01f : INFINITY};
            std::vector<bdpt_vec> a(np), b(np), only_col(np);
            std::vector<float> wa(np), wb(np), only_w(np);
            std::vector<unsigned char> pa(4 * np), pb(4 * np), only_px(4 * np);
            bdpt_cpu_reproject(c, &p, a.data(), wa.data(), pa.data());
            bdpt_cpu_reproject(c, &p, b.data(), wb.data(), pb.data());
            bdpt_cpu_reproject(c, &p, only_col.data(), nullptr, nullptr);
            bdpt_cpu_reproject(c, &p, nullptr, only_w.data(), nullptr);
            bdpt_cpu_reproject(c, &p, nullptr, nullptr, only_px.data());
            bad += memcmp(a.data(), b.data(), sizeof(bdpt_vec) * np) != 0 || pa != pb ||
                   memcmp(wa.data(), wb.data(), sizeof(float) * np) != 0;
            bad += memcmp(a.data(), only_col.data(), sizeof(bdpt_vec) * np) != 0 || pa != only_px ||
                   memcmp(wa.data(), only_w.data(), sizeof(float) * np) != 0;
            for (size_t i = 0; i < np; i++)
                if (wa[i] == (float)cnt[i]) bad += memcmp(&a[i], &in[i], sizeof(bdpt_vec)) != 0;
            if (materials == BDPT_DENOISE_ALL) classify(cam0, W, H, id, pos, wa, cnt, &seen);
            if (materials == BDPT_DENOISE_ALL && k + 1 == cams.size()) {   // the capture stores what was returned
                bdpt_cpu_history_capture(c, &p);
                std::vector<bdpt_vec> hc(np);
                std::vector<float> hm(np);
                bdpt_cpu_history_read(c, hc.data(), hm.data());
                bad += memcmp(hc.data(), a.data(), sizeof(bdpt_vec) * np) != 0 ||
                       memcmp(hm.data(), wa.data(), sizeof(float) * np) != 0;
                bdpt_camera got;
                bad += !bdpt_cpu_history_stored(c, &got) || memcmp(&got, &cams[k], sizeof got) != 0;
            }
        }
        std::vector<bdpt_vec> after(np);
        bdpt_cpu_read_radiance(c, after.data(), nullptr);
        bad += memcmp(after.data(), in.data(), sizeof(bdpt_vec) * np) != 0;   // the accumulation is only read
    }
    printf("%dx%d: took history %d, borders left %d right %d top %d bottom %d, behind the old camera %d, mismatches %d\n",
           W, H, seen.took, seen.left, seen.right, seen.top, seen.bottom, seen.behind, bad);
    bad += !(seen.left && seen.right && seen.top && seen.bottom && seen.behind && seen.took);
    bdpt_cpu_destroy(c);
    return bad;
}

int main(int argc, char** argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: reproject_asan <MersenneTwister.dat>\n");
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
