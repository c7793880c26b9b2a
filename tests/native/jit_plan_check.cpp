// Host check of the specialised-kernel build plan (bdpt_jit_plan.h): the variant index, the
// environment as values, the scene literals, the option strings of every variant, the first attempt
// and the verdict on each build.  Every expected figure is worked out by hand, beside it.
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>
#include "../../gpu_bidirectional_raytracer_amd/csrc/bdpt_jit_plan.h"

static int cases = 0, failed = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        cases++;                                                         \
        if (!(cond)) {                                                   \
            failed++;                                                    \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);       \
        }                                                                \
    } while (0)

typedef std::vector<std::string> strs;

static bool same(const strs& got, const strs& want) {
    if (got == want) return true;
    for (size_t i = 0; i < got.size() || i < want.size(); i++) {
        const char* g = i < got.size() ? got[i].c_str() : "(none)";
        const char* w = i < want.size() ? want[i].c_str() : "(none)";
        if (std::string(g) != w) printf("  option %zu: got %s, want %s\n", i, g, w);
    }
    return false;
}
static strs cat(strs a, const strs& b) {
    a.insert(a.end(), b.begin(), b.end());
    return a;
}

static bdpt_jit_variant variant(int kind, bool pair = true, bool tiles = false) {
    bdpt_jit_variant v;
    v.kind = kind; v.pair = pair; v.tiles = tiles;
    return v;
}
static bdpt_jit_attempt attempt(int waves, bool coarse = false, bool pf_off = false) {
    bdpt_jit_attempt a;
    a.waves = waves; a.coarse = coarse; a.pf_off = pf_off;
    return a;
}
static bdpt_jit_env flags(const char* f) {
    bdpt_jit_env e;
    e.flags = f;
    return e;
}
static bdpt_sphere sphere(float x, float y, float z, float rad, float emit) {
    bdpt_sphere s = {};
    s.rad = rad;
    s.p.x = x; s.p.y = y; s.p.z = z;
    s.e.x = emit;                       // one non-zero component makes an emitter
    return s;
}

// Nine spheres at (i, 0.5, -2) of radius 2, sphere 3 emitting.
static bdpt_jit_scene nine() {
    std::vector<bdpt_sphere> sp;
    for (int i = 0; i < 9; i++) sp.push_back(sphere((float)i, 0.5f, -2.f, 2.f, i == 3 ? 12.f : 0.f));
    return bdpt_jit_scene_of(sp.data(), 9, true);
}
// Hex-float literals: 0.5 = 0x1p-1, -2 = -0x1p+1, rad^2 = 4 = 0x1p+2; x = 0, 1, 2 = 0x1p+1,
// 3 = 1.5 * 2 = 0x1.8p+1, 4 = 0x1p+2, 5 = 1.25 * 4 = 0x1.4p+2, 6 = 0x1.8p+2, 7 = 1.75 * 4 =
// 0x1.cp+2, 8 = 0x1p+3.
#define TAIL ",0x1p-1f,-0x1p+1f,0x1p+2f}"
static const char kNineGeom[] =
    "{{0x0p+0f" TAIL ",{0x1p+0f" TAIL ",{0x1p+1f" TAIL ",{0x1.8p+1f" TAIL ",{0x1p+2f" TAIL
    ",{0x1.4p+2f" TAIL ",{0x1.8p+2f" TAIL ",{0x1.cp+2f" TAIL ",{0x1p+3f" TAIL "}";
// the options every build of that scene starts with: emitter 3 alone is mask 1 << 3 = 8
static strs nine_base(int waves) {
    return {"--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize",
            "-fno-gpu-flush-denormals-to-zero", "-DBDPT_JIT=1", "-DBDPT_JIT_N=9", "-DBDPT_JIT_EMIS=8ull",
            std::string("-DBDPT_JIT_GEOM=") + kNineGeom, "-DBDPT_JIT_ZERO_SAFE=1",
            "-DBDPT_WAVES_PER_SIMD=" + std::to_string(waves)};
}

static void scenes() {
    const bdpt_jit_scene s = nine();
    CHECK(s.n == 9 && s.emis == 8ull && s.n_vac == 8 && s.zero_exit);
    CHECK(s.geom == kNineGeom);
    // lane groups of 2: ceil(8 / 2) = 4 < ceil(9 / 2) = 5 iterations: the list pays
    CHECK(s.vac_list());
    // two spheres, the first emitting: n_vac = 1 is below every group size 2, 4, 8
    const bdpt_sphere two[2] = {sphere(1.f, 1.f, 1.f, 1.f, 1.f), sphere(2.f, 2.f, 2.f, 1.f, 0.f)};
    const bdpt_jit_scene t = bdpt_jit_scene_of(two, 2, false);
    CHECK(t.n == 2 && t.emis == 1ull && t.n_vac == 1 && !t.zero_exit && !t.vac_list());
    CHECK(t.geom == "{{0x1p+0f,0x1p+0f,0x1p+0f,0x1p+0f},{0x1p+1f,0x1p+1f,0x1p+1f,0x1p+0f}}");
    // 16 spheres without an emitter: n_vac = n, so no group size saves an iteration
    std::vector<bdpt_sphere> dark(16, sphere(0.f, 0.f, 0.f, 1.f, 0.f));
    CHECK(!bdpt_jit_scene_of(dark.data(), 16, false).vac_list());
    // 17 spheres, one emitter: groups of 2 need ceil(16 / 2) = 8 < ceil(17 / 2) = 9
    std::vector<bdpt_sphere> more(17, sphere(0.f, 0.f, 0.f, 1.f, 0.f));
    more[16].e.z = 1.f;
    const bdpt_jit_scene m = bdpt_jit_scene_of(more.data(), 17, false);
    CHECK(m.emis == 1ull << 16 && m.n_vac == 16 && m.vac_list());
    // sphere 63 emitting: the mask's top bit
    std::vector<bdpt_sphere> full(64, sphere(0.f, 0.f, 0.f, 1.f, 0.f));
    full[63].e.y = 1.f;
    CHECK(bdpt_jit_scene_of(full.data(), 64, false).emis == 1ull << 63);
    // literals %a cannot print: rad = 2e19 squares to 4e38 > FLT_MAX = 3.4e38, so rad^2 = inf
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const bdpt_sphere odd = sphere(nan, -inf, -0.f, 2e19f, 0.f);
    CHECK(bdpt_jit_scene_of(&odd, 1, false).geom ==
          "{{__builtin_nanf(\"\"),(-__builtin_inff()),-0x0p+0f,__builtin_inff()}}");
    CHECK(bdpt_jit_hexf(inf) == "__builtin_inff()" && bdpt_jit_hexf(-nan) == "__builtin_nanf(\"\")");
    CHECK(bdpt_jit_hexf(0.1f) == "0x1.99999ap-4f");          // 0.1f = 0x3dcccccd = 1.6000000238 / 16
}

static void options() {
    const bdpt_jit_scene s = nine();
    const bdpt_jit_env none;
    // names: the sphere count, then pass streams or not; the tile-list instance has its own
    CHECK(bdpt_jit_name(variant(BDPT_KERNEL_STREAMS), s) == "&bdpt_path_kernel_t<9, true>");
    CHECK(bdpt_jit_name(variant(BDPT_KERNEL_POOL), s) == "&bdpt_path_kernel_t<9, true>");
    CHECK(bdpt_jit_name(variant(BDPT_KERNEL_UNITS), s) == "&bdpt_path_kernel_t<9, true>");
    CHECK(bdpt_jit_name(variant(BDPT_KERNEL_FUSED, false), s) == "&bdpt_path_kernel_t<9, false>");
    CHECK(bdpt_jit_name(variant(BDPT_KERNEL_STREAMS, true, true), s) == "&bdpt_path_tiles_kernel_t<9, true>");
    CHECK(bdpt_jit_name(variant(BDPT_KERNEL_FUSED, true, true), s) == "&bdpt_path_tiles_kernel_t<9, false>");

    // pass streams: the base alone (the VAC list holds, so no -DBDPT_VAC_LIST=0)
    CHECK(same(bdpt_jit_options(variant(BDPT_KERNEL_STREAMS), s, none, attempt(6)), nine_base(6)));
    // `pair` is the fused kernel's: a pass-stream build ignores it
    CHECK(same(bdpt_jit_options(variant(BDPT_KERNEL_STREAMS, false), s, none, attempt(6)), nine_base(6)));
    // fused: its wave count a second time; unpaired: -DBDPT_RNG_PAIR=0 after it
    CHECK(same(bdpt_jit_options(variant(BDPT_KERNEL_FUSED), s, none, attempt(5)),
               cat(nine_base(5), {"-DBDPT_FUSED_WAVES=5"})));
    CHECK(same(bdpt_jit_options(variant(BDPT_KERNEL_FUSED, false), s, none, attempt(5)),
               cat(nine_base(5), {"-DBDPT_FUSED_WAVES=5", "-DBDPT_RNG_PAIR=0"})));
    // pools: never the straight-line part-full rounds
    CHECK(same(bdpt_jit_options(variant(BDPT_KERNEL_POOL), s, none, attempt(6)),
               cat(nine_base(6), {"-DBDPT_POOL=1", "-DBDPT_PF_UNROLL=0"})));
    CHECK(same(bdpt_jit_options(variant(BDPT_KERNEL_UNITS), s, none, attempt(6)),
               cat(nine_base(6), {"-DBDPT_UNITS=1"})));
    CHECK(same(bdpt_jit_options(variant(BDPT_KERNEL_STREAMS, true, true), s, none, attempt(6)),
               cat(nine_base(6), {"-DBDPT_TILES=1"})));
    CHECK(same(bdpt_jit_options(variant(BDPT_KERNEL_FUSED, false, true), s, none, attempt(5)),
               cat(nine_base(5), {"-DBDPT_FUSED_WAVES=5", "-DBDPT_RNG_PAIR=0", "-DBDPT_TILES=1"})));
    // an attempt's own switches: pf_off before the coarse table, which comes last
    CHECK(same(bdpt_jit_options(variant(BDPT_KERNEL_UNITS), s, none, attempt(6, false, true)),
               cat(nine_base(6), {"-DBDPT_UNITS=1", "-DBDPT_PF_UNROLL=0"})));
    CHECK(same(bdpt_jit_options(variant(BDPT_KERNEL_UNITS), s, none, attempt(6, true, true)),
               cat(nine_base(6), {"-DBDPT_UNITS=1", "-DBDPT_PF_UNROLL=0", "-DBDPT_SC_COARSE=1"})));
    // user flags: split on spaces and commas (runs of them too), placed before BDPT_SC_COARSE
    const bdpt_jit_env user = flags(" -DBDPT_A=1,-DBDPT_B  -DBDPT_C=2,, ");
    CHECK(same(user.tokens(), {"-DBDPT_A=1", "-DBDPT_B", "-DBDPT_C=2"}));
    CHECK(same(bdpt_jit_options(variant(BDPT_KERNEL_STREAMS), s, user, attempt(6, true, false)),
               cat(nine_base(6), {"-DBDPT_A=1", "-DBDPT_B", "-DBDPT_C=2", "-DBDPT_SC_COARSE=1"})));
    CHECK(none.tokens().empty() && flags(", ,").tokens().empty());
    // flags that name BDPT_PF_UNROLL decide it: neither the pool build nor pf_off adds =0
    const bdpt_jit_env pf = flags("-DBDPT_PF_UNROLL=1");
    CHECK(pf.pf_user() && !none.pf_user() && !user.pf_user());
    CHECK(same(bdpt_jit_options(variant(BDPT_KERNEL_POOL), s, pf, attempt(6)),
               cat(nine_base(6), {"-DBDPT_POOL=1", "-DBDPT_PF_UNROLL=1"})));
    CHECK(same(bdpt_jit_options(variant(BDPT_KERNEL_STREAMS), s, pf, attempt(6, false, true)),
               cat(nine_base(6), {"-DBDPT_PF_UNROLL=1"})));
    // the two-sphere scene: no VAC list, after the variant's options and before the attempt's
    const bdpt_sphere two[2] = {sphere(1.f, 1.f, 1.f, 1.f, 1.f), sphere(2.f, 2.f, 2.f, 1.f, 0.f)};
    const bdpt_jit_scene t = bdpt_jit_scene_of(two, 2, false);
    CHECK(same(bdpt_jit_options(variant(BDPT_KERNEL_POOL, true, true), t, user, attempt(4, true, false)),
               {"--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize",
                "-fno-gpu-flush-denormals-to-zero", "-DBDPT_JIT=1", "-DBDPT_JIT_N=2", "-DBDPT_JIT_EMIS=1ull",
                "-DBDPT_JIT_GEOM={{0x1p+0f,0x1p+0f,0x1p+0f,0x1p+0f},{0x1p+1f,0x1p+1f,0x1p+1f,0x1p+0f}}",
                "-DBDPT_JIT_ZERO_SAFE=0", "-DBDPT_WAVES_PER_SIMD=4", "-DBDPT_POOL=1", "-DBDPT_TILES=1",
                "-DBDPT_VAC_LIST=0", "-DBDPT_PF_UNROLL=0", "-DBDPT_A=1", "-DBDPT_B", "-DBDPT_C=2",
                "-DBDPT_SC_COARSE=1"}));
}

static void first_attempts() {
    bdpt_jit_env e;
    for (int kind : {BDPT_KERNEL_STREAMS, BDPT_KERNEL_POOL, BDPT_KERNEL_UNITS})
        CHECK(bdpt_jit_first_attempt(variant(kind), e) == attempt(6));
    CHECK(bdpt_jit_first_attempt(variant(BDPT_KERNEL_STREAMS, true, true), e) == attempt(6));
    CHECK(bdpt_jit_first_attempt(variant(BDPT_KERNEL_FUSED), e) == attempt(5));
    CHECK(bdpt_jit_first_attempt(variant(BDPT_KERNEL_FUSED, false, true), e) == attempt(5));
    e.has_waves = true; e.waves = 8;            // BDPT_JIT_WAVES: the pass-stream builds only
    CHECK(bdpt_jit_first_attempt(variant(BDPT_KERNEL_UNITS), e) == attempt(8));
    CHECK(bdpt_jit_first_attempt(variant(BDPT_KERNEL_FUSED), e) == attempt(5));
    e.has_fused_waves = true; e.fused_waves = 4;   // BDPT_JIT_FUSED_WAVES: the fused builds only
    CHECK(bdpt_jit_first_attempt(variant(BDPT_KERNEL_FUSED), e) == attempt(4));
    CHECK(bdpt_jit_first_attempt(variant(BDPT_KERNEL_STREAMS), e) == attempt(8));
    e.waves = 3; e.has_waves = false;           // a value without the variable counts for nothing
    CHECK(bdpt_jit_first_attempt(variant(BDPT_KERNEL_STREAMS), e) == attempt(6));
}

// The attempts a variant goes through when every build reports (stat, scratch) by `report`, from
// the first attempt to the one kept; empty if it does not end within 32 builds.
template <class F>
static std::vector<bdpt_jit_attempt> run(const bdpt_jit_variant& v, const bdpt_jit_scene& s, const bdpt_jit_env& e, F report) {
    std::vector<bdpt_jit_attempt> seq;
    bdpt_jit_attempt a = bdpt_jit_first_attempt(v, e);
    for (int i = 0; i < 32; i++) {
        seq.push_back(a);
        int stat = 0, scratch = 0;
        report(a, &stat, &scratch);
        const bdpt_jit_verdict j = bdpt_jit_judge(v, s, e, a, stat, scratch);
        if (j.keep) return seq;
        a = j.next;
    }
    return {};
}
typedef std::vector<bdpt_jit_attempt> attempts;

static void verdicts() {
    // The LDS estimate for n = 64, bdpt_path_smem(5 n = 320, slots, 0, 0) =
    // 16 * (320 + 3 * slots + 5 + 1024) + 4 * slots:
    //   slots  1 (pass streams):        16 * 1352 +   4 = 21636
    //   slots 16 (units, P <= 16):      16 * 1397 +  64 = 22416
    //   slots 32 (units, P = 32):       16 * 1445 + 128 = 23248
    //   slots 64 (fused, 64 passes):    16 * 1541 + 256 = 24912
    // and fine = 163840 / (dyn + stat), half = 163840 / (dyn + stat - 2048), rounded down.
    CHECK(bdpt_path_smem(320, 1, 0, 0) == 21636 && bdpt_path_smem(320, 16, 0, 0) == 22416);
    CHECK(bdpt_path_smem(320, 32, 0, 0) == 23248 && bdpt_path_smem(320, 64, 0, 0) == 24912);
    std::vector<bdpt_sphere> sp(64, sphere(0.f, 0.f, 0.f, 1.f, 0.f));
    const bdpt_jit_scene big = bdpt_jit_scene_of(sp.data(), 64, false);
    const bdpt_jit_scene small = nine();
    const bdpt_jit_variant st = variant(BDPT_KERNEL_STREAMS), fu = variant(BDPT_KERNEL_FUSED);
    const bdpt_jit_variant po = variant(BDPT_KERNEL_POOL), un = variant(BDPT_KERNEL_UNITS);
    const bdpt_jit_env none;
    bdpt_jit_env ok;
    ok.scratch_ok = true;
    // small static LDS, nine spheres: dyn = 16 * (45 + 3 + 1029) + 4 = 17236, + 4600 = 21836:
    // fine = 7 >= 6 waves, so the coarse test never fires in the spill cases below
    const int kStat = 4600;

    // a clean build is kept as it is
    bdpt_jit_verdict j = bdpt_jit_judge(st, small, none, attempt(6), kStat, 0);
    CHECK(j.keep);
    // spill at 6 -> the same waves without the unrolled rounds; again -> 5, kept even with scratch
    auto spills = [](const bdpt_jit_attempt&, int* stat, int* scratch) { *stat = 4600; *scratch = 64; };
    CHECK(run(st, small, none, spills) == (attempts{attempt(6), attempt(6, false, true), attempt(5, false, true)}));
    CHECK(run(un, small, none, spills) == (attempts{attempt(6), attempt(6, false, true), attempt(5, false, true)}));
    // ... and the build without the unrolled rounds is kept where it does not spill
    auto unrolled_spills = [](const bdpt_jit_attempt& a, int* stat, int* scratch) { *stat = 4600; *scratch = a.pf_off ? 0 : 64; };
    CHECK(run(st, small, none, unrolled_spills) == (attempts{attempt(6), attempt(6, false, true)}));
    // the pool build has no unrolled rounds to drop: straight to 5
    CHECK(run(po, small, none, spills) == (attempts{attempt(6), attempt(5)}));
    // neither when the user's flags name BDPT_PF_UNROLL
    CHECK(run(st, small, flags("-DBDPT_PF_UNROLL=1"), spills) == (attempts{attempt(6), attempt(5)}));
    // BDPT_JIT_SCRATCH_OK keeps the first build, at any wave count
    CHECK(run(st, small, ok, spills) == (attempts{attempt(6)}));
    ok.has_waves = true; ok.waves = 7;           // (21836 B: fine = 7 is not below 7 waves either)
    CHECK(run(st, small, ok, spills) == (attempts{attempt(7)}));
    // an override below the floor is kept with scratch; every start value ends, at min(start, 5)
    // after one same-waves retry above 5: 8 -> 8', 7', 6', 5' (five builds), 6 -> 6', 5' (three).
    // One sphere and no static LDS, so that LDS allows 8 waves of every kind: the fused build's
    // 16 * (5 + 192 + 1029) + 256 = 19872 B give fine = 8 (8.24), the others need less.
    const bdpt_sphere one = sphere(0.f, 0.f, 0.f, 1.f, 0.f);
    const bdpt_jit_scene tiny = bdpt_jit_scene_of(&one, 1, false);
    auto spills0 = [](const bdpt_jit_attempt&, int* stat, int* scratch) { *stat = 0; *scratch = 64; };
    for (int w = 1; w <= 8; w++) {
        bdpt_jit_env e;
        e.has_waves = true; e.waves = w;
        e.has_fused_waves = true; e.fused_waves = w;
        for (const bdpt_jit_variant& v : {st, fu, po, un}) {
            const attempts seq = run(v, tiny, e, spills0);
            const bool retry = w > 5 && !v.pool();
            CHECK(seq.size() == (size_t)(w > 5 ? w - 5 + 1 + (retry ? 1 : 0) : 1));
            CHECK(!seq.empty() && seq.back() == attempt(w > 5 ? 5 : w, false, retry));
        }
    }
    {
        bdpt_jit_env e;
        e.has_waves = true; e.waves = 3;
        CHECK(run(st, small, e, spills) == (attempts{attempt(3)}));
        e.waves = 0;                             // atoi of a word: still at or below the floor
        CHECK(run(st, small, e, spills) == (attempts{attempt(0)}));
    }

    // Coarse trigger, pass streams at 6 waves, n = 64: stat = 6000 -> 27636: fine = 5 (5.93) < 6,
    // half = 163840 / 25588 = 6 (6.40) > 5: the same waves with the 2-KB table, and once only
    j = bdpt_jit_judge(st, big, none, attempt(6), 6000, 0);
    CHECK(!j.keep && j.next == attempt(6, true, false));
    j = bdpt_jit_judge(st, big, none, attempt(6, true, false), 6000 - 2048, 0);
    CHECK(j.keep);
    j = bdpt_jit_judge(st, big, none, attempt(6, true, false), 6000, 0);   // never coarse twice
    CHECK(j.keep);
    auto lds6000 = [](const bdpt_jit_attempt& a, int* stat, int* scratch) { *stat = a.coarse ? 3952 : 6000; *scratch = 0; };
    CHECK(run(st, big, none, lds6000) == (attempts{attempt(6), attempt(6, true, false)}));
    // stat = 8364 -> 30000: fine = 5 (5.46) < 6, but half = 163840 / 27952 = 5 (5.86): no gain
    j = bdpt_jit_judge(st, big, none, attempt(6), 8364, 0);
    CHECK(j.keep);
    // enough LDS for the wave count: stat = 5000 -> 26636: fine = 6 (6.15), not below 6 waves
    j = bdpt_jit_judge(st, big, none, attempt(6), 5000, 0);
    CHECK(j.keep);
    // ... and at 7 waves fine = 6 is below, but half = 163840 / 24588 = 6 (6.66) gains nothing
    j = bdpt_jit_judge(st, big, none, attempt(7), 5000, 0);
    CHECK(j.keep);
    // flags that name BDPT_SC_COARSE decide the table themselves
    CHECK(flags("-DBDPT_SC_COARSE=0").user_coarse() && !none.user_coarse());
    j = bdpt_jit_judge(st, big, flags("-DBDPT_SC_COARSE=0"), attempt(6), 6000, 0);
    CHECK(j.keep);
    // a failed static-LDS query (-1) skips the test; the scratch rules still run
    j = bdpt_jit_judge(st, big, none, attempt(6), -1, 0);
    CHECK(j.keep);
    j = bdpt_jit_judge(st, big, none, attempt(6), -1, 64);
    CHECK(!j.keep && j.next == attempt(6, false, true));
    // both fire: the coarse table first, and the spill is judged on the next build
    j = bdpt_jit_judge(st, big, none, attempt(6), 6000, 64);
    CHECK(!j.keep && j.next == attempt(6, true, false));
    CHECK(run(st, big, none, [](const bdpt_jit_attempt& a, int* stat, int* scratch) { *stat = a.coarse ? 3952 : 6000; *scratch = 64; }) ==
          (attempts{attempt(6), attempt(6, true, false), attempt(6, true, true), attempt(5, true, true)}));
    // fused at 5 waves, 64 pass slots: stat = 8000 -> 32912: fine = 4 (4.98) < 5, half =
    // 163840 / 30864 = 5 (5.31) > 4: coarse; with 32 pass slots dyn = 23248, 31248: fine = 5
    j = bdpt_jit_judge(fu, big, none, attempt(5), 8000, 0);
    CHECK(!j.keep && j.next == attempt(5, true, false));
    bdpt_jit_env e32;
    e32.fused_max_passes = 32;
    j = bdpt_jit_judge(fu, big, e32, attempt(5), 8000, 0);
    CHECK(j.keep);
    // Units stage max(BDPT_UNITS, 16) pass slots.  stat = 5000: one slot gives 26636 (fine 6, kept,
    // above), 16 slots 27416: fine = 5 (5.97) < 6, half = 163840 / 25368 = 6 (6.46): coarse -- for
    // BDPT_UNITS unset (-1), 0, 8 and 16 alike.
    for (int u : {-1, 0, 8, 16}) {
        bdpt_jit_env e;
        e.units = u;
        j = bdpt_jit_judge(un, big, e, attempt(6), 5000, 0);
        CHECK(!j.keep && j.next == attempt(6, true, false));
        // stat = 4500: 16 slots 26916: fine = 6 (6.09): kept
        j = bdpt_jit_judge(un, big, e, attempt(6), 4500, 0);
        CHECK(j.keep);
    }
    // ... where 32 slots give 27748: fine = 5 (5.90), half = 163840 / 25700 = 6 (6.38): coarse
    bdpt_jit_env u32;
    u32.units = 32;
    j = bdpt_jit_judge(un, big, u32, attempt(6), 4500, 0);
    CHECK(!j.keep && j.next == attempt(6, true, false));
    // BDPT_UNITS is the units build's alone: pass streams and pools stage one slot
    j = bdpt_jit_judge(st, big, u32, attempt(6), 5000, 0);
    CHECK(j.keep);
    j = bdpt_jit_judge(po, big, u32, attempt(6), 5000, 0);
    CHECK(j.keep);
}

static void variants() {
    // one memo slot per (kind, tiles, pair), the same every time
    bool seen[kJitVariants] = {};
    int distinct = 0;
    for (int kind : {BDPT_KERNEL_FUSED, BDPT_KERNEL_STREAMS, BDPT_KERNEL_POOL, BDPT_KERNEL_UNITS})
        for (int tiles = 0; tiles < 2; tiles++)
            for (int pair = 0; pair < 2; pair++) {
                const bdpt_jit_variant v = variant(kind, pair != 0, tiles != 0);
                const int i = v.index();
                CHECK(i >= 0 && i < kJitVariants && i == variant(kind, pair != 0, tiles != 0).index());
                if (i >= 0 && i < kJitVariants && !seen[i]) { seen[i] = true; distinct++; }
            }
    CHECK(distinct == 16 && kJitVariants == 16);
    // pinned: ((kind - FUSED) * 2 + tiles) * 2 + pair with FUSED, STREAMS, POOL, UNITS = 1, 2, 3, 4
    CHECK(variant(BDPT_KERNEL_FUSED, false, false).index() == 0 && variant(BDPT_KERNEL_FUSED, true, false).index() == 1);
    CHECK(variant(BDPT_KERNEL_FUSED, true, true).index() == 3 && variant(BDPT_KERNEL_STREAMS, true, false).index() == 5);
    CHECK(variant(BDPT_KERNEL_STREAMS, true, true).index() == 7 && variant(BDPT_KERNEL_POOL, true, false).index() == 9);
    CHECK(variant(BDPT_KERNEL_UNITS, true, false).index() == 13 && variant(BDPT_KERNEL_UNITS, true, true).index() == 15);
    CHECK(variant(BDPT_KERNEL_POOL) == variant(BDPT_KERNEL_POOL, true, false));
    CHECK(!(variant(BDPT_KERNEL_POOL) == variant(BDPT_KERNEL_UNITS)));
    CHECK(!(variant(BDPT_KERNEL_FUSED, true) == variant(BDPT_KERNEL_FUSED, false)));
    CHECK(!(variant(BDPT_KERNEL_STREAMS, true, true) == variant(BDPT_KERNEL_STREAMS, true, false)));
    const bdpt_jit_variant d;                    // the default: the plain pass-stream build
    CHECK(d == variant(BDPT_KERNEL_STREAMS) && d.streams() && !d.pool() && !d.units());
    CHECK(!variant(BDPT_KERNEL_FUSED).streams() && variant(BDPT_KERNEL_POOL).streams() && variant(BDPT_KERNEL_UNITS).streams());
}

static void envs() {
    const bdpt_jit_env a;
    bdpt_jit_env b;
    CHECK(a == b);
    b.units = 8;                                 // the input the old name list had lost
    CHECK(!(a == b));
    b = a; b.flags = "-DBDPT_SREC=0";
    CHECK(!(a == b));
    b = a; b.has_waves = true;                   // set to 0 is not unset
    CHECK(!(a == b));
    b = a; b.waves = 5;
    CHECK(!(a == b));
    b = a; b.has_fused_waves = true;
    CHECK(!(a == b));
    b = a; b.fused_waves = 4;
    CHECK(!(a == b));
    b = a; b.scratch_ok = true;
    CHECK(!(a == b));
    b = a; b.fused_max_passes = 128;
    CHECK(!(a == b));

    // sample records: on unless the last -DBDPT_SREC of the flags says =0
    CHECK(a.srec_enabled());
    CHECK(flags("-DBDPT_PF_UNROLL=0 -DBDPT_IKEY=0").srec_enabled());
    CHECK(flags("-DBDPT_SREC").srec_enabled());
    CHECK(flags("-DBDPT_SREC=1").srec_enabled());
    CHECK(!flags("-DBDPT_SREC=0").srec_enabled());
    CHECK(!flags("-DBDPT_X=1,-DBDPT_SREC=0 -DBDPT_Y").srec_enabled());
    CHECK(flags("-DBDPT_SREC=0 -DBDPT_SREC").srec_enabled());
    CHECK(flags("-DBDPT_SREC=0,-DBDPT_SREC=1").srec_enabled());
    CHECK(!flags("-DBDPT_SREC -DBDPT_SREC=0").srec_enabled());
    CHECK(!flags("-DBDPT_SREC=1 -DBDPT_SREC=0").srec_enabled());
}

// The rules tests/count_scenes.py restates, as a table for tests/test_count_scenes_cpu.py (argument
// "rules"): "vac <n> <n_vac> <vac_list>" for every 0 <= n_vac <= n <= 64 from bdpt_jit_scene, and
// "pf <nl> <lg> <fits> <iters>" for every 1 <= nl <= 64, 1 <= lg <= 5 from the part-full rounds'
// two functions.  Those live in device code; they are quoted here from bdpt_kernels.hip:450 and
// :453 (BDPT_PF_MAX_IT: :124), and the Python test holds the quotation to that file's text.
#define BDPT_PF_MAX_IT 8
constexpr int pf_iters(int nl, int lg) { return (nl + (1 << lg) - 1) >> lg; }
constexpr bool pf_fits(int nl, int lg) { return (1 << (lg - 1)) < nl && pf_iters(nl, lg) <= BDPT_PF_MAX_IT; }

static void rules() {
    for (unsigned n = 1; n <= 64; n++)
        for (unsigned n_vac = 0; n_vac <= n; n_vac++) {
            bdpt_jit_scene s;
            s.n = n;
            s.n_vac = n_vac;
            printf("vac %u %u %d\n", n, n_vac, s.vac_list() ? 1 : 0);
        }
    for (int nl = 1; nl <= 64; nl++)
        for (int lg = 1; lg <= 5; lg++) printf("pf %d %d %d %d\n", nl, lg, pf_fits(nl, lg) ? 1 : 0, pf_iters(nl, lg));
}

int main(int argc, char** argv) {
    if (argc > 1 && std::string(argv[1]) == "rules") {
        rules();
        return 0;
    }
    scenes();
    options();
    first_attempts();
    verdicts();
    variants();
    envs();
    if (failed) {
        printf("%d of %d checks failed\n", failed, cases);
        return 1;
    }
    printf("ok: %d checks\n", cases);
    return 0;
}
