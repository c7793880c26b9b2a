// noise_asan.cpp -- TEST INFRASTRUCTURE: the CPU backend's noise estimate (bdpt_cpu_noise_* and
// bdpt_noise_summarize, csrc/bdpt_cpu.cpp) under AddressSanitizer + UBSan, driven directly with no
// context layer and no Python (`make asan`, run by tests/test_noise_asan.py):
//   noise_asan <MersenneTwister.dat>
// On a 33x9 frame (one tile plus a partial column and row) and a 7x5 frame (one partial tile) of the
// built-in scene: four passes, a mark, four more passes, then estimates into buffers of exactly the
// packed size -- W*H floats, tiles_x*tiles_y floats and counts -- so that a slot outside the frame
// that is read or written is a report.  Then uploaded counters and marks on both sides of the
// fresh-sample rule, at the cap and far above it (counts near 2^32: the integer comparisons must not
// wrap), with and without re-marking.  Checked besides: two calls give the same bytes, each output
// alone equals the joint call, the summary agrees with the per-pixel plane, re-marking leaves the
// estimate it was made with unchanged and moves the mark as the rule says, clearing leaves no valid
// pixel, and the accumulation is only read.  Exit status 0 = clean.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../gpu_bidirectional_raytracer_amd/csrc/bdpt_cpu.h"

struct Result {
    std::vector<float> err, S, E;
    std::vector<unsigned> cv, pend;
    bdpt_noise_summary sum;
};

static Result estimate(bdpt_cpu_ctx* c, int W, int H, const bdpt_noise_params& p) {
    const int tx = (W + BDPT_NOISE_TW - 1) / BDPT_NOISE_TW, ty = (H + BDPT_NOISE_TH - 1) / BDPT_NOISE_TH;
    const size_t np = (size_t)W * H, nt = (size_t)tx * ty;
    Result r{std::vector<float>(np), std::vector<float>(nt), std::vector<float>(nt), std::vector<unsigned>(nt),
             std::vector<unsigned>(nt), {}};
    bdpt_cpu_noise_estimate(c, &p, r.err.data(), r.S.data(), r.E.data(), r.cv.data(), r.pend.data());
    bdpt_noise_summarize(r.S.data(), r.E.data(), r.cv.data(), r.pend.data(), tx, ty, p.threshold, &r.sum);
    return r;
}

static int differ(const Result& a, const Result& b) {
    return memcmp(a.err.data(), b.err.data(), sizeof(float) * a.err.size()) != 0 ||
           memcmp(a.S.data(), b.S.data(), sizeof(float) * a.S.size()) != 0 ||
           memcmp(a.E.data(), b.E.data(), sizeof(float) * a.E.size()) != 0 || a.cv != b.cv || a.pend != b.pend ||
           a.sum.valid_pixels != b.sum.valid_pixels || a.sum.pending_pixels != b.sum.pending_pixels ||
           a.sum.valid_tiles != b.sum.valid_tiles || a.sum.tiles_over != b.sum.tiles_over ||
           memcmp(&a.sum.mean, &b.sum.mean, sizeof(double)) != 0 ||
           memcmp(&a.sum.max_tile, &b.sum.max_tile, sizeof(float)) != 0;
}

// the summary against the per-pixel plane and the counters
static int consistent(const Result& r, const std::vector<unsigned>& cnt) {
    long long valid = 0, pending = 0;
    for (size_t i = 0; i < r.err.size(); i++) {
        const bool ok = r.err[i] >= 0.f || r.err[i] != r.err[i];   // (a NaN is a valid pixel's value)
        valid += ok;
        pending += !ok && cnt[i] > 0u && cnt[i] < BDPT_COUNTER_CAP;
        if (!ok && r.err[i] != -1.0f) return 1;
    }
    return valid != r.sum.valid_pixels || pending != r.sum.pending_pixels;
}

static void passes(bdpt_cpu_ctx* c, bdpt_pass_state* ps, int npass) {
    std::vector<unsigned> sid(npass);
    std::vector<int> vlp(npass);
    bdpt_pass_schedule(ps, npass, sid.data(), vlp.data());
    bdpt_cpu_path_passes(c, sid.data(), vlp.data(), npass);
}

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
    const size_t np = (size_t)W * H;
    const bdpt_noise_params plain = {0.01f, 0.05f, 0}, re = {0.01f, 0.05f, 1};
    int bad = 0;

    // no mark yet: nothing stored, nothing valid, every rendered pixel pending
    passes(c, &ps, 4);
    bad += bdpt_cpu_noise_stored(c);
    std::vector<bdpt_vec> col(np);
    std::vector<unsigned> cnt(np);
    bdpt_cpu_read_radiance(c, col.data(), cnt.data());
    Result r0 = estimate(c, W, H, plain);
    bad += r0.sum.valid_pixels != 0 || r0.sum.pending_pixels != (long long)np || consistent(r0, cnt);
    bad += bdpt_cpu_noise_stored(c);

    // rendered frames: mark at 4 passes, estimate at 8
    bdpt_cpu_noise_mark(c);
    bad += !bdpt_cpu_noise_stored(c);
    passes(c, &ps, 4);
    bdpt_cpu_read_radiance(c, col.data(), cnt.data());
    const Result a = estimate(c, W, H, plain), b = estimate(c, W, H, plain);
    bad += differ(a, b) || consistent(a, cnt) || a.sum.valid_pixels != (long long)np;
    {                                                      // each output alone
        const size_t nt = a.S.size();
        std::vector<float> e(np), S(nt), E(nt);
        std::vector<unsigned> cv(nt), pd(nt);
        bdpt_cpu_noise_estimate(c, &plain, e.data(), nullptr, nullptr, nullptr, nullptr);
        bdpt_cpu_noise_estimate(c, &plain, nullptr, S.data(), nullptr, nullptr, nullptr);
        bdpt_cpu_noise_estimate(c, &plain, nullptr, nullptr, E.data(), nullptr, nullptr);
        bdpt_cpu_noise_estimate(c, &plain, nullptr, nullptr, nullptr, cv.data(), nullptr);
        bdpt_cpu_noise_estimate(c, &plain, nullptr, nullptr, nullptr, nullptr, pd.data());
        bad += memcmp(e.data(), a.err.data(), sizeof(float) * np) != 0 || cv != a.cv || pd != a.pend ||
               memcmp(S.data(), a.S.data(), sizeof(float) * nt) != 0 || memcmp(E.data(), a.E.data(), sizeof(float) * nt) != 0;
    }
    const Result m = estimate(c, W, H, re);                // formed from the old mark, then every pixel re-marks
    bad += differ(a, m);
    std::vector<bdpt_vec> mc(np);
    std::vector<unsigned> mn(np);
    bdpt_cpu_noise_read_mark(c, mc.data(), mn.data());
    bad += memcmp(mc.data(), col.data(), sizeof(bdpt_vec) * np) != 0 || mn != cnt;
    const Result after = estimate(c, W, H, plain);         // cnt == mn now: nothing valid
    bad += after.sum.valid_pixels != 0 || consistent(after, cnt);
    const long long rendered_valid = a.sum.valid_pixels;

    // uploaded counters and marks around every rule
    const unsigned counts[9] = {0u, 1u, 2u, 3u, 4u, 29999u, 30000u, 0xfffffff0u, 0x80000001u};
    long long took = 0;
    for (size_t i = 0; i < np; i++) {
        cnt[i] = counts[i % 9];
        const unsigned k = cnt[i], top = (unsigned)((2ull * k + 2) / 3);
        const unsigned marks[7] = {0u, k, k ? k - 1 : 0u, top, top ? top - 1 : 0u, k / 2, k + 5u};
        mn[i] = marks[(i / 9 + i) % 7];
        mc[i] = {col[i].z, 0.f, -col[i].x};
    }
    bdpt_cpu_write_radiance(c, col.data(), cnt.data());
    bad += bdpt_cpu_noise_stored(c) == false;              // cleared, not forgotten
    bdpt_cpu_noise_read_mark(c, nullptr, mn.data() /* scratch */);
    for (size_t i = 0; i < np; i++) bad += mn[i] != 0u;
    for (size_t i = 0; i < np; i++) {
        const unsigned k = cnt[i], top = (unsigned)((2ull * k + 2) / 3);
        const unsigned marks[7] = {0u, k, k ? k - 1 : 0u, top, top ? top - 1 : 0u, k / 2, k + 5u};
        mn[i] = marks[(i / 9 + i) % 7];
    }
    bdpt_cpu_noise_write_mark(c, mc.data(), mn.data());
    const Result s1 = estimate(c, W, H, plain), s2 = estimate(c, W, H, re);
    bad += differ(s1, s2) || consistent(s1, cnt);
    for (size_t i = 0; i < np; i++) {                      // the fresh-sample rule, in 64 bits
        const bool ok = mn[i] > 0u && cnt[i] > mn[i] && 2ull * (cnt[i] - mn[i]) >= mn[i];
        bad += ok != (s1.err[i] != -1.0f);
    }
    std::vector<bdpt_vec> mc2(np);
    std::vector<unsigned> mn2(np);
    bdpt_cpu_noise_read_mark(c, mc2.data(), mn2.data());
    for (size_t i = 0; i < np; i++) {
        const bool take = cnt[i] > 0u && cnt[i] < BDPT_COUNTER_CAP && (unsigned long long)cnt[i] >= 2ull * mn[i];
        took += take;
        bad += mn2[i] != (take ? cnt[i] : mn[i]);
        bad += memcmp(&mc2[i], take ? &col[i] : &mc[i], sizeof(bdpt_vec)) != 0;
    }
    std::vector<bdpt_vec> now(np);
    bdpt_cpu_read_radiance(c, now.data(), nullptr);
    bad += memcmp(now.data(), col.data(), sizeof(bdpt_vec) * np) != 0;   // the accumulation is only read

    bdpt_cpu_noise_clear(c);
    const Result cleared = estimate(c, W, H, plain);
    bad += cleared.sum.valid_pixels != 0;
    bdpt_cpu_reset_accum(c);
    bdpt_cpu_set_camera(c, &cam);
    bdpt_cpu_set_scene(c, spheres, n);
    printf("%dx%d: tiles %dx%d, rendered valid %lld, uploaded valid %lld pending %lld took the mark %lld, mismatches %d\n",
           W, H, s1.sum.tiles_x, s1.sum.tiles_y, rendered_valid, s1.sum.valid_pixels, s1.sum.pending_pixels, took, bad);
    bad += !(s1.sum.valid_pixels > 0 && s1.sum.pending_pixels > 0 && took > 0);
    bdpt_cpu_destroy(c);
    return bad;
}

int main(int argc, char** argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: noise_asan <MersenneTwister.dat>\n");
        return 2;
    }
    static uint32_t params[4 * BDPT_MT_RNG_COUNT];
    FILE* f = fopen(argv[1], "rb");
    if (!f || fread(params, sizeof params, 1, f) != 1) {
        fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    fclose(f);
    const int bad = run(params, 33, 9) + run(params, 7, 5);
    return bad ? 1 : 0;
}
