// denoise_noise_asan.cpp -- TEST INFRASTRUCTURE: the CPU backend's noise-guided denoiser
// (bdpt_cpu_denoise_noise, csrc/bdpt_cpu.cpp) under AddressSanitizer + UBSan, driven directly with
// no context layer and no Python (`make asan`, run by tests/test_denoise_noise_asan.py):
//   denoise_noise_asan <MersenneTwister.dat>
// On a 33x9 frame and a 7x5 frame of the built-in scene (steps up to 128 reach far outside both):
// four passes, a mark, four more passes, then the filter into buffers of exactly the packed size --
// W*H colours, 4*W*H bytes, W*H floats -- so that a tap outside the frame that is read, or a slot
// outside that is written, is a report.  Then uploaded counters and marks on both sides of the
// validity rule and near 2^32 (the integer comparisons must not wrap).  Checked besides: two calls
// give the same bytes, each output alone equals the joint call, a context without a mark and one
// with a cleared mark give bdpt_cpu_denoise's bytes and no variance, the variance plane has an
// estimate exactly where the definition says one can exist, and the accumulation and the mark are
// only read.  Exit status 0 = clean.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../gpu_bidirectional_raytracer_amd/csrc/bdpt_cpu.h"

struct Out {
    std::vector<bdpt_vec> col;
    std::vector<unsigned char> px;
    std::vector<float> var;
};

static Out filter(const bdpt_cpu_ctx* c, size_t np, const bdpt_denoise_noise_params& p) {
    Out o{std::vector<bdpt_vec>(np), std::vector<unsigned char>(4 * np), std::vector<float>(np)};
    bdpt_cpu_denoise_noise(c, &p, o.col.data(), o.px.data(), o.var.data());
    return o;
}

static int differ(const Out& a, const Out& b) {
    return memcmp(a.col.data(), b.col.data(), sizeof(bdpt_vec) * a.col.size()) != 0 || a.px != b.px ||
           memcmp(a.var.data(), b.var.data(), sizeof(float) * a.var.size()) != 0;
}

// the plain denoiser's bytes and no variance anywhere
static int is_plain(const bdpt_cpu_ctx* c, size_t np, const bdpt_denoise_noise_params& p) {
    const bdpt_denoise_params q = {p.levels, p.normal_power, p.sigma_color, p.materials};
    std::vector<bdpt_vec> col(np);
    std::vector<unsigned char> px(4 * np);
    bdpt_cpu_denoise(c, &q, col.data(), px.data());
    const Out o = filter(c, np, p);
    int bad = memcmp(col.data(), o.col.data(), sizeof(bdpt_vec) * np) != 0 || px != o.px;
    for (size_t i = 0; i < np; i++) bad += o.var[i] != -1.0f;
    return bad;
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
    const bdpt_denoise_noise_params dflt = {4, 5, 0.5f, BDPT_DENOISE_DIFFUSE, 1.0f},
                                    deep = {8, 0, 0.25f, BDPT_DENOISE_ALL, 4.0f},
                                    one = {1, 6, 2.0f, BDPT_DENOISE_ALL, 0.5f};
    const bdpt_denoise_noise_params all[3] = {dflt, deep, one};
    int bad = 0;

    passes(c, &ps, 4);
    for (const auto& p : all) bad += is_plain(c, np, p);   // no mark stored
    bdpt_cpu_noise_mark(c);
    for (const auto& p : all) bad += is_plain(c, np, p);   // marked, no fresh samples: valid nowhere
    passes(c, &ps, 4);
    std::vector<bdpt_vec> col(np), mc(np);
    std::vector<unsigned> cnt(np), mn(np);
    bdpt_cpu_read_radiance(c, col.data(), cnt.data());
    bdpt_cpu_noise_read_mark(c, mc.data(), mn.data());
    long long rendered_est = 0;
    for (const auto& p : all) {
        const Out a = filter(c, np, p), b = filter(c, np, p);
        bad += differ(a, b);
        Out s{std::vector<bdpt_vec>(np), std::vector<unsigned char>(4 * np), std::vector<float>(np)};
        bdpt_cpu_denoise_noise(c, &p, s.col.data(), nullptr, nullptr);   // each output alone
        bdpt_cpu_denoise_noise(c, &p, nullptr, s.px.data(), nullptr);
        bdpt_cpu_denoise_noise(c, &p, nullptr, nullptr, s.var.data());
        bad += differ(a, s);
        if (&p == &all[0])
            for (size_t i = 0; i < np; i++) rendered_est += !(a.var[i] < 0.f);
    }

    // uploaded counters and marks around the rule
    const unsigned counts[9] = {0u, 1u, 2u, 3u, 4u, 29999u, 30000u, 0xfffffff0u, 0x80000001u};
    for (size_t i = 0; i < np; i++) {
        cnt[i] = counts[i % 9];
        mc[i] = {col[i].z, 0.f, -col[i].x};
    }
    bdpt_cpu_write_radiance(c, col.data(), cnt.data());
    for (const auto& p : all) bad += is_plain(c, np, p);   // the upload cleared the mark
    long long valid = 0;
    for (size_t i = 0; i < np; i++) {
        const unsigned k = cnt[i], top = (unsigned)((2ull * k + 2) / 3);
        const unsigned marks[7] = {0u, k, k ? k - 1 : 0u, top, top ? top - 1 : 0u, k / 2, k + 5u};
        mn[i] = marks[(i / 9 + i) % 7];
        valid += mn[i] > 0u && cnt[i] > mn[i] && 2ull * (cnt[i] - mn[i]) >= mn[i];
    }
    bdpt_cpu_noise_write_mark(c, mc.data(), mn.data());
    long long uploaded_est = 0;
    for (const auto& p : all) {
        const Out a = filter(c, np, p), b = filter(c, np, p);
        bad += differ(a, b);
        long long est = 0;
        for (size_t i = 0; i < np; i++) est += !(a.var[i] < 0.f);
        // with ALL every hit pixel near a valid one gets an estimate; none can appear without a valid pixel
        bad += valid == 0 && est != 0;
        if (&p == &all[1]) uploaded_est = est;
    }
    std::vector<bdpt_vec> now(np), mc2(np);
    std::vector<unsigned> cnt2(np), mn2(np);
    bdpt_cpu_read_radiance(c, now.data(), cnt2.data());
    bdpt_cpu_noise_read_mark(c, mc2.data(), mn2.data());
    bad += memcmp(now.data(), col.data(), sizeof(bdpt_vec) * np) != 0 || cnt2 != cnt;   // only read
    bad += memcmp(mc2.data(), mc.data(), sizeof(bdpt_vec) * np) != 0 || mn2 != mn;
    bdpt_cpu_noise_clear(c);
    for (const auto& p : all) bad += is_plain(c, np, p);
    printf("%dx%d: rendered estimates %lld, uploaded valid %lld estimates %lld, mismatches %d\n", W, H, rendered_est,
           valid, uploaded_est, bad);
    bad += !(rendered_est > 0 && valid > 0 && uploaded_est >= valid);
    bdpt_cpu_destroy(c);
    return bad;
}

int main(int argc, char** argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: denoise_noise_asan <MersenneTwister.dat>\n");
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
