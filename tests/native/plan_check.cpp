// Host check of the path-pass planner (bdpt_plan.h): the shard grid, how a call is cut into
// launches and which S it gets, pools and units, the auto stream mode's role sequence and its
// decision, the choice bits and the LDS formula.  Every expected figure is worked out by hand for
// 32 x 8 tiles and 256 compute units; the cut rows agree with launch_passes and Mode.last_streams
// of tests/accum_modes.py.
#include <cstdio>
#include <initializer_list>
#include "../../gpu_bidirectional_raytracer_amd/csrc/bdpt_plan.h"

static int cases = 0, failed = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        cases++;                                                         \
        if (!(cond)) {                                                   \
            failed++;                                                    \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);       \
        }                                                                \
    } while (0)

enum { D = BDPT_CHOICE_DECIDED, F = BDPT_CHOICE_FUSED, P = BDPT_CHOICE_PAIRED, Q = BDPT_CHOICE_QUARTER,
       PO = BDPT_CHOICE_POOLS, U = BDPT_CHOICE_UNITS };

static bdpt_plan_in frame(int W, int H, int streams_req, int npass) {
    bdpt_plan_in in = {W, H, 0, 1, 8, streams_req, npass, 9u, false, BDPT_TRAVERSE_AUTO, 0, 128, 256};
    return in;
}
static bdpt_tuner chosen(int bits) {
    bdpt_tuner t;
    if (bits) t.set_choice(bits);
    return t;
}
// a tuner about to measure `role`
static bdpt_tuner at_role(int role) {
    bdpt_tuner t;
    for (int r = 0; r < role; r++) t.record(r, true, r, 8);
    return t;
}
// `launches` launches, the first of `first` passes, and S (-1: not checked)
static bool cut(const bdpt_plan& p, int npass, int launches, int first, int S) {
    const bdpt_launch l = bdpt_plan_launch(p, 0, npass, false, false, false, false, false, false, 44, 0, bdpt_path_env());
    return p.launches == launches && l.npass == first && (S < 0 || p.S == S);
}

static void shard_grid() {
    static_assert(BDPT_BTW == 32 && BDPT_BTH == 8, "the figures below are for 32 x 8 tiles");
    for (int band : {1, 8, 12, 16}) {
        const bdpt_shard_rows g = bdpt_shard_grid(65, 0, 1, band);
        CHECK(g.grid_rows == 9 && g.tiles_per_band == 0);
    }
    int sum = 0;
    for (int k = 0; k < 3; k++) {
        const bdpt_shard_rows g = bdpt_shard_grid(65, k, 3, 8);
        CHECK(g.grid_rows == 3 && g.tiles_per_band == 1);
        sum += g.grid_rows;
    }
    CHECK(sum == 9);
    // bands of two tile rows: shard 1 owns bands 1 and 4, and the second tile row of band 4 (the
    // frame's last, rows 64..79) lies below the frame
    bdpt_shard_rows g = bdpt_shard_grid(65, 1, 3, 16);
    CHECK(g.grid_rows == 3 && g.tiles_per_band == 2);
    for (int k = 0; k < 3; k++) {
        g = bdpt_shard_grid(65, k, 3, 12);                  // not a whole number of tile rows
        CHECK(g.grid_rows == 9 && g.tiles_per_band == 0);
    }
    g = bdpt_shard_grid(8, 2, 3, 8);                        // one band, three shards: owns nothing
    CHECK(g.grid_rows == 0 && g.tiles_per_band == 1);
    bdpt_plan_in in = frame(97, 8, -1, 20);
    in.shard = 2; in.nshards = 3;
    CHECK(bdpt_plan_call(in, bdpt_tuner(), bdpt_path_env()).launches == 0);
}

static void cut_and_streams() {
    const bdpt_path_env env;
    CHECK(cut(bdpt_plan_call(frame(97, 65, 0, 20), chosen(D), env), 20, 1, 20, 10));
    CHECK(cut(bdpt_plan_call(frame(97, 65, 0, 20), chosen(D | Q), env), 20, 1, 20, 5));
    CHECK(cut(bdpt_plan_call(frame(97, 65, 0, 6), chosen(D | Q), env), 6, 1, 6, 3));   // four per lane need >= 8
    CHECK(cut(bdpt_plan_call(frame(97, 65, -1, 20), chosen(0), env), 20, 1, 20, 20));
    CHECK(cut(bdpt_plan_call(frame(97, 65, 3, 20), chosen(0), env), 20, 1, 20, 3));
    CHECK(cut(bdpt_plan_call(frame(97, 65, 1, 100), chosen(0), env), 100, 2, 50, 1));
    CHECK(cut(bdpt_plan_call(frame(97, 65, -1, 130), chosen(0), env), 130, 2, 65, 65));
    bdpt_path_env lim;
    lim.max_launch_passes = 6;
    CHECK(cut(bdpt_plan_call(frame(97, 65, 0, 20), chosen(D), lim), 20, 4, 5, 3));
    bdpt_plan p = bdpt_plan_call(frame(97, 65, 0, 9), chosen(D | F | P), env);
    CHECK(cut(p, 9, 1, 9, 1) && p.pair);
    p = bdpt_plan_call(frame(97, 65, 0, 9), chosen(D | F), env);
    CHECK(cut(p, 9, 1, 9, 1) && !p.pair);
    // 4097 x 513: 65 tile rows, 2^28 / (65 * 8 * 4097) = 126 passes uncut; equal launches instead
    CHECK(cut(bdpt_plan_call(frame(4097, 513, -1, 128), chosen(0), env), 128, 2, 64, -1));
    p = bdpt_plan_call(frame(97, 65, 0, 20), chosen(D), env);
    CHECK(p.gx == 4 && p.grid_rows == 9 && p.lanes == 9L * 8 * 97 && p.tune_role == -1 && !p.bvh && p.kidx == 9);
    // every launch's S and staged passes: a short last launch gets no idle slices
    p = bdpt_plan_call(frame(97, 65, 3, 7), chosen(0), lim);    // 2 launches: 4 + 3 passes
    CHECK(cut(p, 7, 2, 4, 3));
    const bdpt_launch l1 = bdpt_plan_launch(p, 4, 7, false, false, true, false, true, true, 44, 0, env);
    CHECK(l1.npass == 3 && l1.streams == 3 && l1.st && l1.slots == 1 && l1.kernel == BDPT_KERNEL_STREAMS);
    CHECK(l1.grid[0] == 4 && l1.grid[1] == 9 && l1.grid[2] == 3);
    CHECK(l1.features == (BDPT_FEAT_LAST_SKIP | BDPT_FEAT_STREAMS | BDPT_FEAT_SCP | BDPT_FEAT_SREC |
                          BDPT_FEAT_SPECIALIZED | BDPT_FEAT_DET_SKIP | BDPT_FEAT_ZERO_EXIT));
    const bdpt_launch l2 = bdpt_plan_launch(p, 0, 7, false, false, false, false, false, false, 44, 0, env);
    CHECK(l2.npass == 4 && l2.streams == 3 && l2.slots == 2 && l2.kernel == BDPT_KERNEL_PRECOMPILED);
    CHECK(l2.features == (BDPT_FEAT_LAST_SKIP | BDPT_FEAT_STREAMS | BDPT_FEAT_SCP));
    // the BVH: asked for, or by the auto mode from 128 BVH spheres on
    bdpt_plan_in big = frame(97, 65, 0, 20);
    big.has_bvh = true; big.bvh_ns = 127; big.n_spheres = 200;
    p = bdpt_plan_call(big, chosen(D | Q), env);
    CHECK(!p.bvh && p.kidx == 0 && p.S == 5);
    big.bvh_ns = 128;
    p = bdpt_plan_call(big, chosen(D | Q), env);
    CHECK(p.bvh && p.kidx == 17 && p.S == 20 && !p.quarter_ran);   // one pass per lane under the BVH
}

static void pools_and_units() {
    bdpt_path_env env;
    env.pool = 2;
    bdpt_plan p = bdpt_plan_call(frame(97, 65, -1, 9), chosen(0), env);
    CHECK(p.want_pool && !p.want_units && p.S == 9);
    bdpt_launch l = bdpt_plan_launch(p, 0, 9, true, false, false, false, false, true, 44, 0, env);
    // not overlapped is 64 x 256 pixels per workgroup; overlapped (the default) 128: one workgroup
    // covers the 6984 lanes, rounded up to a group of 8, per pass
    CHECK(l.pooled && l.overlap && l.pool == 2 && l.pool_grid == 128 && l.grid[0] == 8u * 9 && l.grid[1] == 1);
    CHECK(l.kernel == BDPT_KERNEL_POOL && (l.features & BDPT_FEAT_POOLS) && !(l.features & BDPT_FEAT_SCP));
    bdpt_plan_in in = frame(97, 65, -1, 9);
    in.has_bvh = true; in.traversal = BDPT_TRAVERSE_BVH; in.bvh_ns = 30;
    p = bdpt_plan_call(in, chosen(0), env);
    CHECK(p.bvh && !p.want_pool && p.S == 9);
    env = bdpt_path_env();
    env.pool = 0;
    p = bdpt_plan_call(frame(97, 65, 0, 8), at_role(6), env);
    CHECK(p.tune_role == 6 && !p.want_pool && p.S == 4);
    env = bdpt_path_env();
    env.units = 3;
    p = bdpt_plan_call(frame(97, 65, -1, 9), chosen(0), env);
    CHECK(p.want_units && !p.want_pool && p.unit_passes == 3 && p.S == 9);
    for (int taper = 0; taper < 2; taper++) {
        env.units_taper = taper;
        l = bdpt_plan_launch(p, 0, 9, false, true, false, false, true, true, 44, 0, env);
        CHECK(l.unitsl && l.slots == 3 && l.unit_passes == 3 && l.unit_taper == taper);
        CHECK(l.grid[0] == 4u * 9 * (unsigned)bdpt_unit_ranges(9, 3, taper) && l.grid[1] == 1 && l.grid[2] == 1);
        CHECK(l.kernel == BDPT_KERNEL_UNITS && (l.features & BDPT_FEAT_UNITS));
    }
    CHECK(bdpt_unit_ranges(9, 3, 0) == 3 && bdpt_unit_ranges(9, 3, 1) == 4);    // 3 3 3 | 3 3 2 1
    // the measured units need 2 x CUs x 6 tile workgroups: 4 x 9 = 36 < 3072 <= 61 x 136 = 8296
    env = bdpt_path_env();
    bdpt_tuner t = at_role(8);
    p = bdpt_plan_call(frame(97, 65, 0, 8), t, env);
    CHECK(p.tune_role == 8 && !p.want_units && p.S == 4);
    t.record(8, bdpt_role_real(8, p.quarter_ran, true, false, false), 8, 8);
    CHECK(!t.real[8] && t.phase == 9);
    p = bdpt_plan_call(frame(1921, 1081, 0, 8), at_role(8), env);
    CHECK(p.gx == 61 && p.grid_rows == 136 && p.want_units && p.unit_passes == 8 && p.S == 4);
    CHECK(bdpt_plan_call(frame(1921, 1081, 0, 8), chosen(D | U), env).want_units);
    CHECK(!bdpt_plan_call(frame(97, 65, 0, 8), chosen(D | U), env).want_units);
    CHECK(bdpt_plan_call(frame(97, 65, 0, 8), chosen(D | PO), env).want_pool);
}

static void role_sequence() {
    const bdpt_path_env env;
    const int S[10] = {4, 1, 2, 4, 1, 2, 8, 8, 4, 4};
    bdpt_tuner t;
    for (int r = 0; r < 10; r++) {
        CHECK(t.measuring() && !t.decided() && t.choice() == 0 && t.role(8) == r);
        CHECK(t.role(1) == -1);                              // too short to compare
        const bdpt_plan one = bdpt_plan_call(frame(97, 65, 0, 1), t, env);
        CHECK(one.tune_role == -1 && one.S == 1 && t.phase == r);
        const bdpt_plan p = bdpt_plan_call(frame(97, 65, 0, 8), t, env);
        CHECK(p.tune_role == r && p.S == S[r] && p.pair == (r != 4));
        CHECK(p.quarter_ran == (r == 2 || r == 5) && p.want_pool == (r == 6 || r == 7) && !p.want_units);
        t.record(r, bdpt_role_real(r, p.quarter_ran, true, p.want_pool, p.want_units), 100 + r, 8);
        CHECK(t.call[r] == 100 + r && t.npass[r] == 8 && t.real[r] == (r < 8));
    }
    CHECK(!t.measuring() && !t.decided() && t.role(8) == -1 && t.choice() == 0);
    t.decide();
    CHECK(t.decided() && (t.choice() & D));
    t.reset();
    CHECK(t.measuring() && t.role(8) == 0 && t.choice() == 0);
    bdpt_tuner off;                                          // BDPT_STREAMS_TUNE=0: two passes per lane
    off.enabled = false;
    const bdpt_plan p = bdpt_plan_call(frame(97, 65, 0, 8), off, env);
    CHECK(off.role(8) == -1 && p.tune_role == -1 && p.S == 4 && !p.want_pool);
    // which roles are real: role 1 always, role 4 only as a specialised build
    CHECK(bdpt_role_real(1, false, false, false, false) && !bdpt_role_real(4, true, false, true, true));
    CHECK(bdpt_role_real(0, false, false, false, false) && bdpt_role_real(3, false, false, false, false));
    CHECK(!bdpt_role_real(2, false, true, true, true) && bdpt_role_real(5, true, false, false, false));
    CHECK(!bdpt_role_real(7, true, true, false, true) && bdpt_role_real(9, false, false, false, true));
}

static bdpt_tuner measured(const double* ms, const bool* real, int npass) {
    bdpt_tuner t;
    for (int r = 0; r < 10; r++) {
        t.record(r, real[r], r, npass);
        t.set_ms(r, ms[r]);
    }
    return t;
}

static void decision() {
    const bool all[10] = {true, true, true, true, true, true, true, true, true, true};
    // per pass: half 1.0, quarter 0.9, pooled 0.925, units 0.875, fused paired 1.25, unpaired 1.225
    const double ms[10] = {4.0, 5.0, 3.6, 4.2, 4.9, 3.8, 3.7, 3.9, 3.5, 3.65};
    bdpt_tuner t = measured(ms, all, 4);
    t.decide();
    CHECK(t.choice() == (D | Q | U));
    const bool some[10] = {true, true, false, true, false, false, false, false, false, false};
    const double a[10] = {2.0, 1.8, 0.1, 2.2, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1};   // an unreal role never wins
    t = measured(a, some, 2);
    t.decide();
    CHECK(t.choice() == (D | F | P));                        // 0.9 x 1.05 < 1.0
    const double b[10] = {2.0, 1.92, 0.1, 2.2, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1};
    t = measured(b, some, 2);
    t.decide();
    CHECK(t.choice() == (D | P));                            // 0.96 x 1.05 = 1.008 is not below 1.0
    const double pools[10] = {4.0, 5.0, 3.6, 4.2, 4.9, 3.8, 3.4, 3.9, 3.5, 3.65};   // pooled 0.85 now leads
    t = measured(pools, all, 4);
    t.decide();
    CHECK(t.choice() == (D | Q | PO));
}

static void choice_bits() {
    for (int bits = 0; bits < 64; bits++) {
        if (!(bits & D) || ((bits & PO) && (bits & U))) continue;
        bdpt_tuner t;
        t.enabled = false;                                   // a forced choice turns the auto mode on
        t.set_choice(bits);
        CHECK(t.decided() && t.enabled && t.choice() == bits);
        bdpt_tuner peer = at_role(10);
        peer.adopt(t);
        CHECK(peer.decided() && peer.choice() == bits);
    }
}

static void lds() {
    CHECK(bdpt_path_tab(false, 9, 8, 0) == 44 && bdpt_path_tab(true, 200, 190, 6) == 6);
    CHECK(bdpt_path_smem(bdpt_path_tab(false, 9, 8, 0), 10, 0, 0) == 16 * (44 + 30 + 5 + 1024) + 4 * 10);
    CHECK(bdpt_path_smem(44, 10, 0, 0) == 17688);
    CHECK(bdpt_path_smem(5 * 64, 1, 0, 0) == 16 * (320 + 3 + 5 + 1024) + 4);    // the JIT estimate, n = 64
    CHECK(bdpt_path_smem(5 * 64, 1, 0, 0) == 21636);
    CHECK(bdpt_path_smem(6, 2, 6, 256) == 16 * (6 + 6 + 5 + 1024) + 4 * 8 + 256);
    const bdpt_path_env env;
    const bdpt_plan p = bdpt_plan_call(frame(97, 65, 0, 20), chosen(D), env);
    const bdpt_launch l = bdpt_plan_launch(p, 0, 20, false, false, true, false, true, true, 44, 0, env);
    CHECK(l.streams == 10 && l.slots == 2 && l.smem == 16 * (44 + 6 + 5 + 1024) + 4 * 2);
    // static LDS counts: 17688 dynamic + 6152 static fit 23840 exactly and no less
    CHECK(bdpt_path_lds_fits(17688, 6152, 23840) && !bdpt_path_lds_fits(17688, 6152, 23839));
    CHECK(bdpt_path_lds_fits(160 * 1024, 0, 160 * 1024) && !bdpt_path_lds_fits(160 * 1024, 8, 160 * 1024));
    // the largest brute-force scene: one emitter, 2 staged passes, 160 KiB, by hand:
    // 163840 - 6152 static - 16 * (6 + 5 + 1024) - 8 = 141120 = 16 * 8820; 5 n - 1 <= 8820 -> n = 1764
    CHECK(bdpt_path_max_spheres(1, 2, 0, 6152, 160 * 1024) == 1764);
    for (size_t stat : {(size_t)0, (size_t)2056, (size_t)6152, (size_t)8200})
        for (size_t slots : {(size_t)1, (size_t)2, (size_t)128})
            for (size_t ne : {(size_t)0, (size_t)1, (size_t)3}) {
                const size_t lim = 160 * 1024, n = bdpt_path_max_spheres(ne, slots, 0, stat, lim);
                CHECK(n > 1500 && n < 1900);
                CHECK(bdpt_path_lds_fits(bdpt_path_smem(bdpt_path_tab(false, n, n - ne, 0), slots, 0, 0), stat, lim));
                CHECK(!bdpt_path_lds_fits(bdpt_path_smem(bdpt_path_tab(false, n + 1, n + 1 - ne, 0), slots, 0, 0), stat, lim));
            }
    CHECK(bdpt_path_max_spheres(0, 1, 0, 160 * 1024, 160 * 1024) == 0);      // nothing fits
    // the BVH kernel stages the brute-force list and its ids: 16 + 4 bytes per entry
    CHECK(bdpt_path_smem(bdpt_path_tab(true, 5000, 4990, 40), 1, 40, 0) == 16 * (40 + 3 + 5 + 1024) + 4 * 41);
}

int main() {
    shard_grid();
    cut_and_streams();
    pools_and_units();
    role_sequence();
    decision();
    choice_bits();
    lds();
    if (failed) return 1;
    printf("ok %d cases\n", cases);
    return 0;
}
