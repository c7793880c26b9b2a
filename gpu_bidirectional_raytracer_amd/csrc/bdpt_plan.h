// bdpt_plan.h -- what a bdpt_path_passes call launches: the shard's grid, how the call is cut into
// launches, the kernel mode of each launch and the auto stream mode's measurement.  Integer logic
// only: no HIP call, no environment read and no context, so tests/native/plan_check.cpp checks it
// on a machine without a GPU.  bdpt_host.cpp reads the environment into bdpt_path_env, asks for a
// plan and issues what the plan says.
#ifndef BDPT_PLAN_H
#define BDPT_PLAN_H

#include <stddef.h>

#include <algorithm>
#include <limits>

#include "../../include/bdpt.h"
#include "bdpt_device.h"       // BDPT_BTW, BDPT_BTH, bdpt_unit_ranges

// The environment switches the planner reads, as values (bdpt_host.cpp path_env fills them).
struct bdpt_path_env {
    int pool = -1;               // BDPT_POOL: -1 = measured, 0 = never, R > 0 = always, chunks of R x 64 pixels
    int units = -1;              // BDPT_UNITS: -1 = measured, 0 = never, P > 0 = always, ranges of P passes
    int max_launch_passes = 0;   // BDPT_MAX_LAUNCH_PASSES (experiments: smaller launches); < 1 = no limit
    int fused_max_passes = 64;   // BDPT_FUSED_MAX_PASSES, 1..128
    bool pool_overlap = true;    // BDPT_POOL_OVERLAP
    int units_taper = 1;         // BDPT_UNITS_TAPER
    int pool_grid = 0;           // BDPT_POOL_GRID: G x 64 pixels per wave and pass, 1..256; 0 = by shape
    int smem_pad = 0;            // BDPT_SMEM_PAD (experiments: cap workgroups per CU), bytes
};

// The auto stream mode (bdpt_set_streams 0): the first kRoles calls of >= 2 passes each run one
// role of the table below; then the per-pass times decide which variant later calls run.  The
// pass-stream variant kept is the one with the fastest call; the faster fused variant replaces it
// only if it beats that by kMargin.  Calls are compared per pass by path-kernel time plus a quarter
// of the call's fold: the fold runs on its own stream beside the next call's kernels (bdpt_host.cpp
// fold_timing).  Every variant is measured twice except the fused ones, so a cold first call --
// clocks still ramping -- does not decide.  Reset by scene / shard / traversal / specialisation /
// stream-mode changes.  BDPT_STREAMS_TUNE=0 (enabled = false): no measurement, two passes per lane.
// (5 %: open scenes gain >= 10 % from the fused kernel, closed ones lose >= 7 %; with 2 % a
// one-call measurement once kept the fused kernel for gantz, 7 % slower, profiles/r03_s27_*.
// Four passes per lane: cornell_glass / cornell_mirror +1.2 %, synthetic64 -2.8 % at 128-pass
// launches, profiles/r03_s45_ab_passes_per_lane.txt -- so it is measured, not fixed.)
enum bdpt_role_kind {
    BDPT_ROLE_HALF,             // pass streams, two passes per lane
    BDPT_ROLE_FUSED_PAIRED,     // the fused S = 1 kernel, paired segment loads (bdpt_kernels.hip BDPT_RNG_PAIR)
    BDPT_ROLE_QUARTER,          // pass streams, four passes per lane (launches of >= 8 passes)
    BDPT_ROLE_FUSED_UNPAIRED,   // the fused kernel without pairing (a specialised build only)
    BDPT_ROLE_POOLS,            // pass streams with pixel pools (specialised builds only, BDPT_POOL)
    BDPT_ROLE_UNITS,            // pass streams with the ordered in-kernel fold (specialised builds of
                                // shards with enough tile workgroups, BDPT_UNITS)
    BDPT_ROLE_KINDS
};
constexpr int kTuneRoles = 10;
constexpr bdpt_role_kind kTuneRole[kTuneRoles] = {
    BDPT_ROLE_HALF,  BDPT_ROLE_FUSED_PAIRED,   BDPT_ROLE_QUARTER,       // roles 0, 1, 2
    BDPT_ROLE_HALF,  BDPT_ROLE_FUSED_UNPAIRED, BDPT_ROLE_QUARTER,       // roles 3, 4, 5
    BDPT_ROLE_POOLS, BDPT_ROLE_POOLS,          BDPT_ROLE_UNITS, BDPT_ROLE_UNITS};   // roles 6 .. 9
// Whether a tuning call really ran its role's variant, from what the call launched: otherwise the
// role repeated another role's kernel and must not decide anything.  Four passes per lane need
// launches of >= 8 passes, and the unpaired fused variant, the pools and the units exist only as
// specialised builds.
inline bool bdpt_role_real(int role, bool quarter_ran, bool fused_specialized, bool pool_ran, bool units_ran) {
    switch (kTuneRole[role]) {
    case BDPT_ROLE_QUARTER: return quarter_ran;
    case BDPT_ROLE_FUSED_UNPAIRED: return fused_specialized;
    case BDPT_ROLE_POOLS: return pool_ran;
    case BDPT_ROLE_UNITS: return units_ran;
    default: return true;
    }
}

struct bdpt_tuner {
    static constexpr double kMargin = 0.05;
    bool enabled = true;
    int phase = 0;                  // < kTuneRoles: the next role; kTuneRoles: all issued; + 1: decided
    // the decision
    bool fused = false;
    bool pair = true;               // the fused variant kept: paired segment loads or not
    bool quarter = false;           // the pass-stream variant kept: four passes per lane,
    bool pool = false;              // pixel pools,
    bool units = false;             // or the ordered in-kernel fold
    // per role: the call that measured it, its time, whether it ran its variant, its passes
    long long call[kTuneRoles] = {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1};
    double ms[kTuneRoles] = {};
    bool real[kTuneRoles] = {};
    int npass[kTuneRoles] = {};

    bool measuring() const { return phase < kTuneRoles; }
    bool decided() const { return phase == kTuneRoles + 1; }
    void reset() {                  // measure again
        const bool e = enabled;
        *this = bdpt_tuner();
        enabled = e;
    }
    int choice() const {            // BDPT_CHOICE_* bits; 0 while there is no decision
        if (!enabled || !decided()) return 0;
        return BDPT_CHOICE_DECIDED | (fused ? BDPT_CHOICE_FUSED : 0) | (pair ? BDPT_CHOICE_PAIRED : 0) |
               (quarter ? BDPT_CHOICE_QUARTER : 0) | (pool ? BDPT_CHOICE_POOLS : 0) | (units ? BDPT_CHOICE_UNITS : 0);
    }
    void set_choice(int bits) {     // a decision made elsewhere (bits checked by the caller)
        fused = (bits & BDPT_CHOICE_FUSED) != 0;
        pair = (bits & BDPT_CHOICE_PAIRED) != 0;
        quarter = (bits & BDPT_CHOICE_QUARTER) != 0;
        pool = (bits & BDPT_CHOICE_POOLS) != 0;
        units = (bits & BDPT_CHOICE_UNITS) != 0;
        enabled = true;
        phase = kTuneRoles + 1;
    }
    void adopt(const bdpt_tuner& leader) { set_choice(leader.choice()); }
    // the role a call of npass passes measures, or -1 (not measuring, or a call too short to compare)
    int role(int npass) const { return enabled && measuring() && npass >= 2 ? phase : -1; }
    void record(int role, bool ran, long long call_no, int passes) {
        real[role] = ran;
        call[role] = call_no;
        npass[role] = passes;
        phase = role + 1;
    }
    void set_ms(int role, double t) { ms[role] = t; }
    void decide() {                 // after every role's call has been timed
        double best[BDPT_ROLE_KINDS];
        for (double& b : best) b = std::numeric_limits<double>::infinity();
        for (int r = 0; r < kTuneRoles; r++)
            if (real[r]) best[kTuneRole[r]] = std::min(best[kTuneRole[r]], ms[r] / npass[r]);
        const double half = best[BDPT_ROLE_HALF], qu = best[BDPT_ROLE_QUARTER], pooled = best[BDPT_ROLE_POOLS];
        const double un = best[BDPT_ROLE_UNITS], fp = best[BDPT_ROLE_FUSED_PAIRED], fn = best[BDPT_ROLE_FUSED_UNPAIRED];
        pair = !(fn < fp);          // the default unless unpaired was measured faster
        quarter = qu < half;
        pool = pooled < std::min(half, qu) && !(un < pooled);
        units = un < std::min(std::min(half, qu), pooled);
        const double streams = std::min(std::min(std::min(half, qu), pooled), un);
        fused = (pair ? fp : fn) * (1.0 + kMargin) < streams;
        phase = kTuneRoles + 1;
    }
};

// Grid rows of a shard: every tile row, or (bands a whole number of tile rows) only this shard's
// bands.  tiles_per_band > 0: the grid rows enumerate only the shard's bands (bdpt_dev_tile_row).
struct bdpt_shard_rows { int grid_rows, tiles_per_band; };
inline bdpt_shard_rows bdpt_shard_grid(int H, int shard, int nshards, int band_rows) {
    const int tile_rows = (H + BDPT_BTH - 1) / BDPT_BTH;
    if (nshards <= 1 || band_rows % BDPT_BTH != 0) return {tile_rows, 0};
    const int tpb = band_rows / BDPT_BTH;
    const int nbands = (H + band_rows - 1) / band_rows;
    const int owned = shard < nbands ? (nbands - shard + nshards - 1) / nshards : 0;
    int grid_rows = owned * tpb;
    // only the frame's last band can be partial: launch none of its tile rows below the frame
    if (owned > 0) {
        const int last = shard + (owned - 1) * nshards;      // this shard's last band
        const int tail = (last + 1) * tpb - tile_rows;
        if (tail > 0) grid_rows -= tail;
    }
    return {grid_rows, tpb};
}

constexpr int kUnitPasses = 8;   // passes per unit range in the auto mode (profiles/r05_s5_*)

struct bdpt_plan_in {
    int W, H, shard, nshards, band_rows;
    int streams_req;                // bdpt_set_streams: 0 = auto (measured), -1 = one pass per lane
    int npass;
    unsigned n_spheres;
    bool has_bvh;
    int traversal, bvh_ns, bvh_auto_spheres;   // BDPT_TRAVERSE_*, BVH spheres, the auto mode's threshold
    int cus;
    // bdpt_path_passes_tiles: the mask's non-zero bytes, or -1 for a call without a mask.  A masked
    // call launches one workgroup per listed tile and stream, never pools or units, and takes no
    // part in the auto mode's measurement (it follows the decision kept, and leaves it alone).
    int ntiles = -1;
};

struct bdpt_plan {
    int gx, grid_rows, tiles_per_band;   // tile columns and rows of a launch
    int ntiles;                     // >= 0: the launch enumerates a list of this many tiles of the gx x grid_rows grid
    long lanes;                     // launched pixels per pass (a listed tile counts in full: 256)
    int chunk;                      // passes per launch (the last may have fewer)
    int launches;
    int S;                          // pass streams of a full launch (bdpt_last_streams)
    bool pair;                      // fused kernel: paired segment loads
    int tune_role;                  // the role this call measures, or -1
    bool bvh;
    int kidx;                       // bdpt_path_kernel_table column
    bool quarter_ran, want_pool, want_units;
    int unit_passes;
};

inline bdpt_plan bdpt_plan_call(const bdpt_plan_in& in, const bdpt_tuner& t, const bdpt_path_env& env) {
    bdpt_plan p{};
    const bdpt_shard_rows rows = bdpt_shard_grid(in.H, in.shard, in.nshards, in.band_rows);
    p.gx = (in.W + BDPT_BTW - 1) / BDPT_BTW;
    p.grid_rows = rows.grid_rows;
    p.tiles_per_band = rows.tiles_per_band;
    // Pass streams: auto = one pass per lane (S = the launch's pass count).  Eye paths are capped
    // at 7 segments and most reach the cap, so single-path lanes keep a wave almost perfectly
    // balanced, while a lane that regenerates through many passes waits for the wave's slowest
    // sum (+11.7 % at 1080p, and it fills the GPU when a shard has few pixels).
    p.lanes = (long)p.grid_rows * BDPT_BTH * in.W;
    const bool listed = in.ntiles >= 0;
    p.ntiles = listed ? in.ntiles : -1;
    if (listed) p.lanes = 256L * in.ntiles;
    int S = in.streams_req <= 0 ? BDPT_MAX_STREAMS : in.streams_req;
    // auto: a measuring call runs its role's variant, later calls the variant kept
    const bool autom = in.streams_req == 0;
    const bool kept = autom && t.enabled && t.decided();
    p.tune_role = autom && !listed ? t.role(in.npass) : -1;
    const int kind = p.tune_role >= 0 ? (int)kTuneRole[p.tune_role] : -1;
    p.pair = true;
    if (kind == BDPT_ROLE_FUSED_PAIRED || kind == BDPT_ROLE_FUSED_UNPAIRED) {
        S = 1;
        p.pair = kind != BDPT_ROLE_FUSED_UNPAIRED;
    } else if (kind < 0 && kept && t.fused) {
        S = 1;
        p.pair = t.pair;
    }
    // keep single launches bounded (~2^28 samples, <= 128 passes for the LDS pass tables)
    const long per_pass = p.lanes > 0 ? p.lanes : 1;
    int chunk = (int)((1L << 28) / per_pass);
    if (chunk < 1) chunk = 1;
    if (chunk > 128) chunk = 128;
    if (env.max_launch_passes >= 1 && env.max_launch_passes < chunk) chunk = env.max_launch_passes;
    if (S > chunk) S = chunk;
    if (S > in.npass) S = in.npass;
    if (S < 1) S = 1;
    if (S == 1 && chunk > env.fused_max_passes) chunk = env.fused_max_passes;   // fused: LDS per pass
    // equal launches: 128 passes over a 4097 x 513-row band (chunk 126) are 2 x 64, not 126 + 2
    if (in.npass > chunk) {
        const int nch = (in.npass + chunk - 1) / chunk;
        chunk = (in.npass + nch - 1) / nch;
        if (S > chunk) S = chunk;
    }
    p.chunk = chunk;
    p.launches = p.grid_rows > 0 && in.ntiles != 0 ? (in.npass + chunk - 1) / chunk : 0;
    p.bvh = in.has_bvh && (in.traversal == BDPT_TRAVERSE_BVH ||
                           (in.traversal == BDPT_TRAVERSE_AUTO && in.bvh_ns >= in.bvh_auto_spheres));
    p.kidx = p.bvh ? 17 : (in.n_spheres <= 16 ? (int)in.n_spheres : 0);
    // auto: the pass-stream kernel renders two passes per lane in launches of >= 4 passes (lanes
    // whose first path ends early start the second in groups, bdpt_kernels.hip BDPT_REGEN_STREAMS):
    // cornell +0.6 %, cornell_glass +1.7 %, cornell_mirror +1.5 %; not for BVH traversal
    // (complex -4.6 %: its lanes' traversal costs differ more than their path lengths)
    // (four passes per lane when the measurement chose them, or to measure them; launches of >= 8)
    if (autom && S >= 4 && !p.bvh) {
        const bool quarter = kind >= 0 ? kind == BDPT_ROLE_QUARTER : (kept && t.quarter);
        p.quarter_ran = quarter && S >= 8;
        S = p.quarter_ran ? (S + 3) / 4 : (S + 1) / 2;
    }
    // pixel pools: forced by BDPT_POOL=R, or measured and kept
    // (a tile list takes neither pools, which enumerate row-major pixels, nor units, whose handover
    // waits are not worth carrying onto a partial tile set -- not even when forced)
    p.want_pool = !listed && !p.bvh && S > 1 && env.pool != 0 &&
                  (env.pool > 0 || (autom && (kind >= 0 ? kind == BDPT_ROLE_POOLS : (kept && t.pool))));
    if (p.want_pool) S = chunk < in.npass ? chunk : in.npass;    // one pass per lane slice
    // ordered in-kernel fold (units of a tile and a range of passes; no radiance buffer): forced by
    // BDPT_UNITS=P (ranges of P passes), or measured and kept; not for shards whose tile workgroups
    // cannot keep the chip busy with one range per tile (a tile's units run one after another)
    const bool units_fit = (long)p.gx * p.grid_rows >= 2L * in.cus * 6;
    p.want_units = !listed && !p.bvh && S > 1 && !p.want_pool && env.units != 0 &&
                   (env.units > 0 ||
                    (autom && units_fit && (kind >= 0 ? kind == BDPT_ROLE_UNITS : (kept && t.units))));
    p.unit_passes = env.units > 0 ? env.units : kUnitPasses;
    p.S = S;
    return p;
}

// Launch shape of a pooled launch of nloc pixels per pass: {chunk R, grid G} (a wave claims R x 64
// pixels at a time; a pass has nloc / (256 G) workgroups).  With the sparse serial fold and
// overlapped launches, larger chunks and grids measured best (profiles/r05_s44_pool_shape.txt,
// r05_s45_*, r05_s46_*, r05_s48_*, r05_s49_*; interleaved rounds, ms per step): whole frame
// (2.08 M) G = 128, R = 64 3.54-3.55 against G = 64, R = 16 3.66-3.68; 1/2 share G = 128, R = 32
// 1.88-1.89 against 1.95-1.96; 1/4 share 0.943-0.954 against 0.956-0.962; 1/8 share (260 K)
// G = 128, R = 16 0.548-0.553 against G = 64, R = 16 0.567-0.568 and G = 128, R = 32 0.576-0.578.
// Launches that are not overlapped (the auto-tuner's calls, BDPT_POOL_OVERLAP=0) keep the shape
// that measured best before the overlap, G = 64, R = 16: a serial launch pays the large shapes'
// drain in full, and with them the tuner's pooled call at the 1/8 share lost to S = 32
// (r05_s50_strong.txt, N = 8 row).
inline void bdpt_pool_shape(long nloc, bool overlap, const bdpt_path_env& env, int* R, int* G) {
    const int r = !overlap ? 16 : nloc >= 1500000 ? 64 : (nloc >= 400000 ? 32 : 16);
    *G = env.pool_grid >= 1 ? env.pool_grid : (overlap ? 128 : 64);
    *R = env.pool > 0 ? env.pool : r;
}

// Pooled launches overlap: each runs (with its fold) on its own stream, so a launch's drain --
// ~0.1 ms at its end, when all passes' pools run out together and the last paths finish at
// falling occupancy -- overlaps the next launch's start (caustic8 +1.1 to +1.7 %, its 1/4 and
// 1/8 shares +4 to +6 %, profiles/r05_s37_pool_overlap.txt).  Not in the stream mode's tuning
// calls (measured one at a time, as the other modes); BDPT_POOL_OVERLAP=0 turns it off.
inline bool bdpt_plan_overlap(const bdpt_plan& p, const bdpt_path_env& env, bool have_pool) {
    return have_pool && env.pool_overlap && p.tune_role < 0;
}

// Dynamic LDS of a path-kernel workgroup: the scene table of `tab` float4 (4 per sphere + the
// non-emitters' list, or a BVH scene's brute-force spheres) + a VLP per staged pass + camera + 4 wave
// shadow queues (results written over maxt) + a sid per staged pass + `ids` brute-force ids (+ a pad).
inline size_t bdpt_path_smem(size_t tab, size_t slots, size_t ids, int pad) {
    return 16 * (tab + 3 * slots + 5 + 4 * 128 * 2) + sizeof(unsigned) * (slots + ids) + (size_t)pad;
}
inline size_t bdpt_path_tab(bool bvh, size_t n, size_t n_vac, size_t big_n) {
    return bvh ? big_n : 4 * n + n_vac;
}
// A workgroup's LDS is the launch's dynamic part (bdpt_path_smem) plus what the kernel declares
// itself (`stat`: the camera basis, the sincos table, the claim words; the launched function's
// HIP_FUNC_ATTRIBUTE_SHARED_SIZE_BYTES): the launch fits when the sum is within the device's
// limit per workgroup.  A launch that does not fit fails in the runtime, so the host refuses it.
inline bool bdpt_path_lds_fits(size_t dyn, size_t stat, size_t limit) { return dyn + stat <= limit; }
// The largest scene the brute-force kernels take: n spheres of which n_emit emit (the non-emitters'
// list has n - n_emit entries), `slots` staged passes; 0 when not even an empty table fits.
inline size_t bdpt_path_max_spheres(size_t n_emit, size_t slots, int pad, size_t stat, size_t limit) {
    const size_t fixed = bdpt_path_smem(0, slots, 0, pad) + stat;
    if (fixed > limit) return 0;
    return ((limit - fixed) / 16 + n_emit) / 5;          // 16 B x (4 n + n - n_emit) <= limit - fixed
}

// Which kernel a launch runs: the precompiled instance or one of the specialised builds.
enum bdpt_launch_kernel {
    BDPT_KERNEL_PRECOMPILED, BDPT_KERNEL_FUSED, BDPT_KERNEL_STREAMS, BDPT_KERNEL_POOL, BDPT_KERNEL_UNITS,
    BDPT_KERNEL_KINDS
};
struct bdpt_launch {
    int npass;                      // passes [p0, p0 + npass) of the call
    int streams;                    // S of this launch: a short last launch gets no idle stream slices
    bool st, pooled, unitsl;        // the pass-stream kernel; its pixel-pool build; its in-kernel fold build
    bool overlap;                   // a pooled launch on its own stream (bdpt_plan_overlap)
    int unit_passes, unit_taper, nranges;   // unitsl: passes per range, halving tail, ranges of the launch
    int pool, pool_grid;            // pooled: {R, G} of bdpt_pool_shape
    size_t slots;                   // passes whose VLP and sid a workgroup stages (bdpt_kernels.hip nslot)
    size_t smem;
    int kernel;                     // bdpt_launch_kernel
    int features;                   // BDPT_FEAT_*
    unsigned grid[3];               // tiles x rows x streams, or 1-D for pools and units
};

// The launch of passes [p0, ...) of a planned call, given which specialised kernels resolved
// (have_*), whether the pass-stream build reads sample records, whether the specialised builds
// have the black-surface exit, and the LDS table terms of the scene (bdpt_path_tab, ids).
inline bdpt_launch bdpt_plan_launch(const bdpt_plan& p, int p0, int npass, bool have_pool, bool have_units,
                                    bool have_streams, bool have_fused, bool use_srec, bool zero_exit,
                                    size_t tab, size_t ids, const bdpt_path_env& env) {
    bdpt_launch l{};
    l.npass = npass - p0 < p.chunk ? npass - p0 : p.chunk;
    l.streams = p.S < l.npass ? p.S : l.npass;
    l.st = l.streams > 1;
    l.pooled = l.st && have_pool;
    l.unitsl = l.st && have_units;
    l.overlap = l.pooled && bdpt_plan_overlap(p, env, have_pool);
    if (l.unitsl) l.unit_passes = p.unit_passes < l.npass ? p.unit_passes : l.npass;
    // a workgroup stages the VLPs and sids of its own passes only
    l.slots = l.unitsl ? (size_t)l.unit_passes : ((size_t)l.npass + l.streams - 1) / l.streams;
    l.smem = bdpt_path_smem(tab, l.slots, ids, env.smem_pad);
    l.kernel = !l.st ? (have_fused ? BDPT_KERNEL_FUSED : BDPT_KERNEL_PRECOMPILED)
               : l.pooled ? BDPT_KERNEL_POOL
               : l.unitsl ? BDPT_KERNEL_UNITS
               : have_streams ? BDPT_KERNEL_STREAMS : BDPT_KERNEL_PRECOMPILED;
    l.features = BDPT_FEAT_LAST_SKIP | (p.bvh ? BDPT_FEAT_BVH : 0) | (l.st ? BDPT_FEAT_STREAMS : 0) |
                 (l.pooled ? BDPT_FEAT_POOLS : 0) | (l.unitsl ? BDPT_FEAT_UNITS : 0) |
                 (l.st && !l.pooled ? BDPT_FEAT_SCP : 0) | (l.st && use_srec ? BDPT_FEAT_SREC : 0) |
                 (l.kernel != BDPT_KERNEL_PRECOMPILED
                      ? BDPT_FEAT_SPECIALIZED | BDPT_FEAT_DET_SKIP | (zero_exit ? BDPT_FEAT_ZERO_EXIT : 0) : 0) |
                 (p.ntiles >= 0 ? BDPT_FEAT_TILES : 0);
    l.grid[0] = (unsigned)p.gx; l.grid[1] = (unsigned)p.grid_rows; l.grid[2] = (unsigned)l.streams;
    if (p.ntiles >= 0) { l.grid[0] = (unsigned)p.ntiles; l.grid[1] = 1; }   // one workgroup per listed tile
    if (l.pooled) {
        // waves of pool x 64 pixels; 1-D, passes interleaved in groups of 8 workgroups (bdpt_kernels.hip s0)
        bdpt_pool_shape(p.lanes, l.overlap, env, &l.pool, &l.pool_grid);
        const long span = 256L * l.pool_grid, per = ((p.lanes + span - 1) / span + 7) / 8 * 8;
        l.grid[0] = (unsigned)(per * l.streams); l.grid[1] = l.grid[2] = 1;
    }
    if (l.unitsl) {
        // one workgroup per unit (tile, range); the last passes in halving ranges (bdpt_device.h
        // bdpt_unit_range), BDPT_UNITS_TAPER=0 off
        l.unit_taper = env.units_taper;
        l.nranges = bdpt_unit_ranges(l.npass, l.unit_passes, l.unit_taper);
        l.grid[0] = (unsigned)(p.gx * p.grid_rows * l.nranges); l.grid[1] = l.grid[2] = 1;
    }
    return l;
}

#endif
