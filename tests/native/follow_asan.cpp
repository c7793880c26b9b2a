// follow_asan.cpp -- TEST INFRASTRUCTURE: the CPU backend's sphere-following history
// (bdpt_cpu_history_follow / bdpt_cpu_history_motion and the reprojection, capture and preview with
// it, csrc/bdpt_cpu.cpp) under AddressSanitizer + UBSan, driven directly with no context layer and
// no Python (`make asan`, run by tests/test_follow_asan.py):
//   follow_asan <MersenneTwister.dat>
// On a 7x5 and a 40x33 frame of the built-in scene, with its two balls made diffuse and the last
// two spheres swapped so that the last index is a ball and not the emitter: four passes and a
// capture, then for each edit the edited spheres, one pass, and reprojection, preview and capture
// into buffers of exactly the packed size -- a read outside the table of offsets or outside [H][W] is
// a report.  The edits:
//   * a ball moved sideways (state 2; its pixels take history that the unfollowed call refuses);
//   * the last sphere moved (the table's last entry is the one gathered);
//   * both moved, and a wall moved (every pixel of it shifted);
//   * refused scenes: the emitter moved, a radius changed, a sphere fewer -- state 3, the frame
//     comes back as it is and the delta buffer is left alone.
// Checked besides: two calls give the same bytes, follow off returns the input, the capture stores
// what the reprojection returned and brings the state back to 1.  Exit status 0 = clean.
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

struct Edit {
    const char* what;
    int state;                  // the state expected
    int moved[2];               // spheres moved by (5, 0, -3), -1: none
    int emitter, radius, fewer; // the refused edits
};

static int run(const uint32_t* params, int W, int H) {
    bdpt_camera cam;
    bdpt_sphere base[9];
    const unsigned n = bdpt_default_scene(&cam, base);
    base[6].refl = base[7].refl = BDPT_DIFF;
    const bdpt_sphere ball = base[7];
    base[7] = base[8];                                    // the emitter
    base[8] = ball;                                       // the last index: a ball
    bdpt_update_camera(&cam, W, H);
    const size_t np = (size_t)W * H;
    int bad = 0, followed = 0, last_followed = 0;
    const Edit edits[] = {
        {"a ball moved", BDPT_HISTORY_MOVED, {6, -1}, 0, 0, 0},
        {"the last sphere moved", BDPT_HISTORY_MOVED, {8, -1}, 0, 0, 0},
        {"both balls moved", BDPT_HISTORY_MOVED, {6, 8}, 0, 0, 0},
        {"a wall moved", BDPT_HISTORY_MOVED, {2, -1}, 0, 0, 0},
        {"the emitter moved", BDPT_HISTORY_UNUSABLE, {6, -1}, 1, 0, 0},
        {"a radius changed", BDPT_HISTORY_UNUSABLE, {-1, -1}, 0, 1, 0},
        {"a sphere fewer", BDPT_HISTORY_UNUSABLE, {-1, -1}, 0, 0, 1},
    };
    for (const Edit& e : edits) {
        bdpt_cpu_ctx* c = bdpt_cpu_create(base, n, W, H, params);
        if (!c) return 1;
        bdpt_cpu_set_camera(c, &cam);
        bdpt_cpu_light_pass(c, 0);
        bdpt_pass_state ps;
        bdpt_pass_state_init(&ps);
        bdpt_pass_state_light(&ps);
        passes(c, &ps, 4);
        const bdpt_reproject_params p = {BDPT_DENOISE_DIFFUSE, 64.f, 0.01f};
        bad += bdpt_cpu_history_motion(c, nullptr) != BDPT_HISTORY_NONE;
        bdpt_cpu_history_capture(c, &p);
        bad += bdpt_cpu_history_motion(c, nullptr) != BDPT_HISTORY_SAME;

        std::vector<bdpt_sphere> s(base, base + n);
        for (int k : e.moved)
            if (k >= 0) {
                s[k].p.x += 5.f;
                s[k].p.z -= 3.f;
            }
        if (e.emitter) s[7].p.y -= 2.f;
        if (e.radius) s[6].rad *= 1.5f;
        if (e.fewer) s.pop_back();
        bdpt_cpu_set_scene(c, s.data(), (unsigned)s.size());
        bdpt_cpu_reset_accum(c);
        bdpt_cpu_light_pass(c, 0);
        bdpt_pass_state_light(&ps);
        passes(c, &ps, 1);

        // the state and the offsets, into a buffer of exactly one entry per sphere
        std::vector<bdpt_vec> delta(s.size(), bdpt_vec{7.f, 7.f, 7.f});
        const int state = bdpt_cpu_history_motion(c, delta.data());
        bad += state != e.state;
        for (size_t k = 0; k < s.size(); k++) {
            const bool is_moved = (int)k == e.moved[0] || (int)k == e.moved[1];
            const bdpt_vec want = state != BDPT_HISTORY_MOVED ? bdpt_vec{7.f, 7.f, 7.f}
                                  : is_moved                  ? bdpt_vec{5.f, 0.f, -3.f}
                                                              : bdpt_vec{0.f, 0.f, 0.f};
            bad += memcmp(&delta[k], &want, sizeof want) != 0;
        }

        std::vector<bdpt_vec> in(np), off(np), a(np), b(np), pv(np);
        std::vector<unsigned> cnt(np);
        std::vector<float> woff(np), wa(np), wb(np), wpv(np);
        std::vector<unsigned char> pa(4 * np), pb(4 * np);
        std::vector<int> id(np);
        bdpt_aov_buffers g;
        memset(&g, 0, sizeof g);
        g.id = id.data();
        bdpt_cpu_render_aov(c, 0, 0, W, H, 0, 0u, &g);
        bdpt_cpu_read_radiance(c, in.data(), cnt.data());
        // follow off: absent, the input comes back
        bad += bdpt_cpu_history_present(c);
        bdpt_cpu_reproject(c, &p, off.data(), woff.data(), nullptr);
        bad += memcmp(off.data(), in.data(), sizeof(bdpt_vec) * np) != 0;
        for (size_t i = 0; i < np; i++) bad += woff[i] != (float)cnt[i];
        // follow on
        bdpt_cpu_history_follow(c, 1);
        bad += bdpt_cpu_history_present(c) != (e.state == BDPT_HISTORY_MOVED);
        bdpt_cpu_reproject(c, &p, a.data(), wa.data(), pa.data());
        bdpt_cpu_reproject(c, &p, b.data(), wb.data(), pb.data());
        bad += memcmp(a.data(), b.data(), sizeof(bdpt_vec) * np) != 0 || pa != pb ||
               memcmp(wa.data(), wb.data(), sizeof(float) * np) != 0;
        const bdpt_preview_params pp = {p, 2, 5, 0.5f, 8.f};
        bdpt_cpu_preview_denoise(c, &pp, pv.data(), wpv.data(), nullptr);
        int took = 0;
        for (size_t i = 0; i < np; i++) {
            const bool on_moved = id[i] >= 0 && (id[i] == e.moved[0] || id[i] == e.moved[1]);
            if (wa[i] == (float)cnt[i]) bad += memcmp(&a[i], &in[i], sizeof(bdpt_vec)) != 0;   // no history: the input's bits
            if (e.state == BDPT_HISTORY_MOVED && on_moved && wa[i] > (float)cnt[i]) {
                took++;
                if (id[i] == 8) last_followed++;
            }
            if (e.state != BDPT_HISTORY_MOVED) bad += wa[i] != (float)cnt[i];
        }
        followed += took;
        // the capture stores what was returned; in state 2 the current spheres become the key
        bdpt_cpu_history_capture(c, &p);
        std::vector<bdpt_vec> hc(np);
        std::vector<float> hm(np);
        bdpt_cpu_history_read(c, hc.data(), hm.data());
        bad += memcmp(hc.data(), a.data(), sizeof(bdpt_vec) * np) != 0 || memcmp(hm.data(), wa.data(), sizeof(float) * np) != 0;
        bad += bdpt_cpu_history_motion(c, delta.data()) != BDPT_HISTORY_SAME;
        std::vector<bdpt_vec> after(np);
        bdpt_cpu_read_radiance(c, after.data(), nullptr);
        bad += memcmp(after.data(), in.data(), sizeof(bdpt_vec) * np) != 0;   // the accumulation is only read
        printf("%dx%d %s: state %d, moved-sphere pixels with history %d, mismatches so far %d\n", W, H, e.what, state,
               took, bad);
        bdpt_cpu_destroy(c);
    }
    printf("%dx%d: followed %d, through the last entry %d, mismatches %d\n", W, H, followed, last_followed, bad);
    bad += !(followed > 0 && last_followed > 0);
    return bad;
}

int main(int argc, char** argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: follow_asan <MersenneTwister.dat>\n");
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
