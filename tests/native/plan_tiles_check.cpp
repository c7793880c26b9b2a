// Host check of the path-pass planner (bdpt_plan.h) for masked calls (bdpt_path_passes_tiles): a
// call planned from the count of listed tiles -- its grid and lanes, the cut into launches, that it
// never takes pixel pools or the units fold, that it measures no role of the auto stream mode and
// follows the decision kept, and that an empty list launches nothing.  Every expected figure is
// worked out by hand for 32 x 8 tiles; 97 x 65 is 4 x 9 = 36 tiles.
#include <cstdio>
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

static bdpt_plan_in frame(int W, int H, int streams_req, int npass, int ntiles) {
    bdpt_plan_in in = {W, H, 0, 1, 8, streams_req, npass, 9u, false, BDPT_TRAVERSE_AUTO, 0, 128, 256};
    in.ntiles = ntiles;
    return in;
}
static bdpt_tuner chosen(int bits) {
    bdpt_tuner t;
    if (bits) t.set_choice(bits);
    return t;
}
static bdpt_tuner at_role(int role) {
    bdpt_tuner t;
    for (int r = 0; r < role; r++) t.record(r, true, r, 8);
    return t;
}
static bdpt_launch first(const bdpt_plan& p, int npass, bool have_streams = false, bool have_fused = false) {
    return bdpt_plan_launch(p, 0, npass, false, false, have_streams, have_fused, have_streams, have_streams, 44, 0,
                            bdpt_path_env());
}

static void grid_and_lanes() {
    const bdpt_path_env env;
    // the default field value is "no mask": the plan of bdpt_path_passes
    bdpt_plan_in plain = {97, 65, 0, 1, 8, -1, 20, 9u, false, BDPT_TRAVERSE_AUTO, 0, 128, 256};
    CHECK(plain.ntiles == -1);
    bdpt_plan p = bdpt_plan_call(plain, chosen(0), env);
    CHECK(p.ntiles == -1 && p.lanes == 9L * 8 * 97 && !(first(p, 20).features & BDPT_FEAT_TILES));
    CHECK(first(p, 20).grid[0] == 4 && first(p, 20).grid[1] == 9 && first(p, 20).grid[2] == 20);
    // 18 of the 36 tiles, one pass per lane: 18 x 1 x 20 workgroups, 256 lanes per tile
    p = bdpt_plan_call(frame(97, 65, -1, 20, 18), chosen(0), env);
    CHECK(p.ntiles == 18 && p.gx == 4 && p.grid_rows == 9 && p.tiles_per_band == 0);
    CHECK(p.lanes == 256L * 18 && p.launches == 1 && p.chunk == 128 && p.S == 20 && p.tune_role == -1);
    bdpt_launch l = first(p, 20);
    CHECK(l.grid[0] == 18 && l.grid[1] == 1 && l.grid[2] == 20 && l.npass == 20 && l.streams == 20);
    CHECK(l.features == (BDPT_FEAT_LAST_SKIP | BDPT_FEAT_STREAMS | BDPT_FEAT_SCP | BDPT_FEAT_TILES));
    l = first(p, 20, true);
    CHECK(l.kernel == BDPT_KERNEL_STREAMS && (l.features & BDPT_FEAT_TILES) && (l.features & BDPT_FEAT_SPECIALIZED));
    // every tile listed: partial edge tiles count in full, more lanes than the unmasked 9 x 8 x 97
    p = bdpt_plan_call(frame(97, 65, 3, 20, 36), chosen(0), env);
    CHECK(p.lanes == 9216 && p.lanes > 9L * 8 * 97 && p.S == 3 && first(p, 20).grid[0] == 36 && first(p, 20).grid[2] == 3);
    // the fused kernel: 36 x 1 x 1
    p = bdpt_plan_call(frame(97, 65, 1, 9, 36), chosen(0), env);
    l = first(p, 9, false, true);
    CHECK(p.S == 1 && l.grid[0] == 36 && l.grid[1] == 1 && l.grid[2] == 1 && !l.st && l.kernel == BDPT_KERNEL_FUSED);
    CHECK((l.features & BDPT_FEAT_TILES) && !(l.features & BDPT_FEAT_STREAMS));
    // the BVH: its kernel column, one pass per lane in auto mode
    bdpt_plan_in big = frame(97, 65, 0, 20, 7);
    big.has_bvh = true; big.bvh_ns = 128; big.n_spheres = 200;
    p = bdpt_plan_call(big, chosen(D | Q), env);
    CHECK(p.bvh && p.kidx == 17 && p.S == 20 && (first(p, 20).features & BDPT_FEAT_BVH) && first(p, 20).grid[0] == 7);
    // an empty list: nothing to launch, whatever the rest says
    p = bdpt_plan_call(frame(97, 65, -1, 20, 0), chosen(0), env);
    CHECK(p.launches == 0 && p.lanes == 0);
}

static void cut() {
    const bdpt_path_env env;
    // 4097 x 513: 129 x 65 = 8385 tiles, 2146560 lanes; 2^28 / 2146560 = 125 passes uncut, so 128
    // passes are two equal launches of 64
    bdpt_plan p = bdpt_plan_call(frame(4097, 513, -1, 128, 8385), chosen(0), env);
    CHECK(p.lanes == 2146560 && p.launches == 2 && p.chunk == 64 && p.S == 64);
    // ... and with one tile in 64 listed (131 tiles) one launch of 128
    p = bdpt_plan_call(frame(4097, 513, -1, 128, 131), chosen(0), env);
    CHECK(p.launches == 1 && p.chunk == 128 && p.S == 128);
    // the 128-pass cap and the fused kernel's 64: 130 = 2 x 65, fused 100 = 2 x 50
    p = bdpt_plan_call(frame(97, 65, -1, 130, 18), chosen(0), env);
    CHECK(p.launches == 2 && p.chunk == 65 && p.S == 65);
    p = bdpt_plan_call(frame(97, 65, 1, 100, 18), chosen(0), env);
    CHECK(p.launches == 2 && p.chunk == 50 && p.S == 1);
    // BDPT_MAX_LAUNCH_PASSES = 6: 20 passes in 4 launches of 5; two per lane: S = 3
    bdpt_path_env lim;
    lim.max_launch_passes = 6;
    p = bdpt_plan_call(frame(97, 65, 0, 20, 18), chosen(D), lim);
    CHECK(p.launches == 4 && p.chunk == 5 && p.S == 3 && !p.quarter_ran);
    const bdpt_launch last = bdpt_plan_launch(p, 15, 20, false, false, false, false, false, false, 44, 0, lim);
    CHECK(last.npass == 5 && last.streams == 3 && last.slots == 2 && last.grid[0] == 18 && last.grid[2] == 3);
    p = bdpt_plan_call(frame(97, 65, 0, 20, 18), chosen(D | F | P), lim);
    CHECK(p.launches == 4 && p.chunk == 5 && p.S == 1 && p.pair);
}

static void no_pools_no_units() {
    for (int streams_req : {-1, 0}) {
        bdpt_path_env env;
        env.pool = 2;
        bdpt_plan p = bdpt_plan_call(frame(97, 65, streams_req, 9, 18), chosen(0), env);
        CHECK(!p.want_pool && !p.want_units);
        CHECK(bdpt_plan_call(frame(97, 65, streams_req, 9, -1), chosen(0), env).want_pool);    // unmasked: forced
        env = bdpt_path_env();
        env.units = 3;
        p = bdpt_plan_call(frame(97, 65, streams_req, 9, 18), chosen(0), env);
        CHECK(!p.want_pool && !p.want_units);
        CHECK(bdpt_plan_call(frame(97, 65, streams_req, 9, -1), chosen(0), env).want_units);
    }
    const bdpt_path_env env;
    // a kept decision for pools or units: a masked call runs plain pass streams, two per lane
    bdpt_plan p = bdpt_plan_call(frame(1921, 1081, 0, 8, 8296), chosen(D | U), env);
    CHECK(!p.want_units && !p.want_pool && p.S == 4);
    CHECK(bdpt_plan_call(frame(1921, 1081, 0, 8, -1), chosen(D | U), env).want_units);
    p = bdpt_plan_call(frame(97, 65, 0, 8, 18), chosen(D | PO), env);
    CHECK(!p.want_pool && p.S == 4);
    // even with the launch's features asked from a resolved pool / units build: never reported
    const bdpt_launch l = bdpt_plan_launch(p, 0, 8, false, false, true, false, true, true, 44, 0, env);
    CHECK(!(l.features & (BDPT_FEAT_POOLS | BDPT_FEAT_UNITS)) && (l.features & BDPT_FEAT_TILES));
}

static void tuner_untouched() {
    const bdpt_path_env env;
    static const int S_unmasked[kTuneRoles] = {4, 1, 2, 4, 1, 2, 8, 8, 4, 4};
    for (int r = 0; r < kTuneRoles; r++) {
        const bdpt_tuner t = at_role(r);
        // while measuring: no role, two passes per lane whatever the role in turn would run
        const bdpt_plan m = bdpt_plan_call(frame(97, 65, 0, 8, 18), t, env);
        CHECK(m.tune_role == -1 && m.S == 4 && m.pair && !m.quarter_ran && !m.want_pool && !m.want_units);
        CHECK(t.phase == r && t.measuring() && t.role(8) == r && t.choice() == 0);
        // the unmasked call after it still measures role r
        const bdpt_plan u = bdpt_plan_call(frame(97, 65, 0, 8, -1), t, env);
        CHECK(u.tune_role == r && u.S == S_unmasked[r]);
    }
    // the decision kept is followed: fused (paired or not), two or four passes per lane
    bdpt_plan p = bdpt_plan_call(frame(97, 65, 0, 20, 18), chosen(D | F | P), env);
    CHECK(p.S == 1 && p.pair && p.tune_role == -1);
    p = bdpt_plan_call(frame(97, 65, 0, 20, 18), chosen(D | F), env);
    CHECK(p.S == 1 && !p.pair);
    p = bdpt_plan_call(frame(97, 65, 0, 20, 18), chosen(D), env);
    CHECK(p.S == 10 && !p.quarter_ran);
    p = bdpt_plan_call(frame(97, 65, 0, 20, 18), chosen(D | Q), env);
    CHECK(p.S == 5 && p.quarter_ran);
    p = bdpt_plan_call(frame(97, 65, 0, 6, 18), chosen(D | Q), env);      // four per lane need >= 8
    CHECK(p.S == 3 && !p.quarter_ran);
    // tuning off (BDPT_STREAMS_TUNE=0): two per lane
    bdpt_tuner off;
    off.enabled = false;
    CHECK(bdpt_plan_call(frame(97, 65, 0, 8, 18), off, env).S == 4);
    // explicit stream counts are honoured
    CHECK(bdpt_plan_call(frame(97, 65, 3, 20, 18), chosen(0), env).S == 3);
    CHECK(bdpt_plan_call(frame(97, 65, -1, 20, 18), chosen(0), env).S == 20);
}

int main() {
    grid_and_lanes();
    cut();
    no_pools_no_units();
    tuner_untouched();
    if (failed) return 1;
    printf("ok %d cases\n", cases);
    return 0;
}
