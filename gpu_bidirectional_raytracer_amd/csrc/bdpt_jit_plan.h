// bdpt_jit_plan.h -- what the run-time compile of a scene-specialised path kernel builds: which
// variant, from which environment switches and scene, with which options, and what to try next
// when a build costs a workgroup of LDS or spills.  Values and pure functions only: no GPU runtime
// call, no environment read and no context, so tests/native/jit_plan_check.cpp checks it on a
// machine without a GPU.  bdpt_jit.cpp reads the environment into bdpt_jit_env, compiles what
// bdpt_jit_options says and asks bdpt_jit_judge about each build.
#ifndef BDPT_JIT_PLAN_H
#define BDPT_JIT_PLAN_H

#include <cmath>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "bdpt_plan.h"          // BDPT_KERNEL_*, bdpt_path_smem

// Which specialised build: the kernel kind (BDPT_KERNEL_FUSED / STREAMS / POOL / UNITS), paired
// segment loads (the fused kernel only: the other kinds ignore it) and the tile-list code.
struct bdpt_jit_variant {
    int kind = BDPT_KERNEL_STREAMS;
    bool pair = true;
    bool tiles = false;

    bool streams() const { return kind != BDPT_KERNEL_FUSED; }   // pools and units are pass-stream builds
    bool pool() const { return kind == BDPT_KERNEL_POOL; }
    bool units() const { return kind == BDPT_KERNEL_UNITS; }
    int index() const { return ((kind - BDPT_KERNEL_FUSED) * 2 + (tiles ? 1 : 0)) * 2 + (pair ? 1 : 0); }
    bool operator==(const bdpt_jit_variant& o) const { return kind == o.kind && pair == o.pair && tiles == o.tiles; }
};
constexpr int kJitVariants = (BDPT_KERNEL_KINDS - BDPT_KERNEL_FUSED) * 4;   // bdpt_jit_variant::index() < this

// Every environment input of a build, by value (bdpt_jit.cpp jit_env fills them): two of these that
// compare equal give the same builds for the same scene and variant.
struct bdpt_jit_env {
    std::string flags;               // BDPT_JIT_FLAGS (experiments: extra -D options); "" = unset
    bool has_waves = false, has_fused_waves = false;   // BDPT_JIT_WAVES / BDPT_JIT_FUSED_WAVES are set,
    int waves = 0, fused_waves = 0;                    // and their values
    bool scratch_ok = false;         // BDPT_JIT_SCRATCH_OK is set: keep a spilling build (experiments)
    int units = -1;                  // BDPT_UNITS as the planner reads it (bdpt_path_env::units)
    int fused_max_passes = 64;       // bdpt_path_env::fused_max_passes

    bool mentions(const char* name) const { return strstr(flags.c_str(), name) != nullptr; }
    bool user_coarse() const { return mentions("BDPT_SC_COARSE"); }   // the flags decide the sincos table
    bool pf_user() const { return mentions("BDPT_PF_UNROLL"); }       // ... the part-full rounds
    // Whether the pass-stream builds have sample records (BDPT_SREC of the kernel source, on by default
    // in these builds): the last -DBDPT_SREC[=v] of the flags decides, and the host must hand a
    // build without them the sin/cos planes.
    bool srec_enabled() const {
        bool on = true;
        const char* f = flags.c_str();
        for (const char* q = strstr(f, "-DBDPT_SREC"); q; q = strstr(q + 1, "-DBDPT_SREC")) {
            const char* v = q + strlen("-DBDPT_SREC");
            on = *v == '=' ? atoi(v + 1) != 0 : true;
        }
        return on;
    }
    // the flags as options: split on spaces and commas, empty tokens dropped
    std::vector<std::string> tokens() const {
        std::vector<std::string> out;
        std::string tok;
        for (const char* q = flags.c_str();; q++) {
            if (*q == ' ' || *q == ',' || *q == 0) {
                if (!tok.empty()) out.push_back(tok);
                tok.clear();
                if (!*q) break;
            } else {
                tok += *q;
            }
        }
        return out;
    }
    bool operator==(const bdpt_jit_env& o) const {
        return flags == o.flags && has_waves == o.has_waves && waves == o.waves &&
               has_fused_waves == o.has_fused_waves && fused_waves == o.fused_waves &&
               scratch_ok == o.scratch_ok && units == o.units && fused_max_passes == o.fused_max_passes;
    }
};

inline std::string bdpt_jit_hexf(float v) {     // exact float literal
    // %a prints "inf" / "nan", which are no literals: rad * rad overflows from rad = 1.85e19 on
    if (std::isinf(v)) return v < 0.f ? "(-__builtin_inff())" : "__builtin_inff()";
    if (v != v) return "__builtin_nanf(\"\")";
    char b[48];
    snprintf(b, sizeof b, "%af", (double)v);
    return b;
}

// The scene as the build folds it in (BDPT_JIT of the kernel source): 1 <= n <= 64 spheres (the emitter
// mask is 64 bits), the geometry {p, rad^2} as exact literals, the black-surface exit and the
// length of the non-emitters' list.
struct bdpt_jit_scene {
    unsigned n = 0;
    unsigned long long emis = 0;     // bit i: sphere i emits
    std::string geom;                // "{{px,py,pz,rr},...}"
    bool zero_exit = false;          // BDPT_ZERO_EXIT is compiled in
    unsigned n_vac = 0;              // non-emitters

    // VLP-only part-full shadow rounds over the non-emitters' list (BDPT_VAC_LIST): only where
    // dropping the emitters saves a lane-group iteration (cornell: 8 of 9 spheres fit 4, 2, 1
    // iterations instead of 5, 3, 2); elsewhere the staging costs (synthetic64 -0.4 %,
    // profiles/r06_s24_ab_vac_list.txt)
    bool vac_list() const {
        for (unsigned k = 1; k <= 3; k++)
            if ((1u << k) <= n_vac && (n_vac + (1u << k) - 1) >> k < (n + (1u << k) - 1) >> k) return true;
        return false;
    }
};
// zero_exit_safe: bdpt_zero_exit_safe of the same spheres (ending a path at a black non-emitter is
// provably exact for this scene, bdpt_util.c).
inline bdpt_jit_scene bdpt_jit_scene_of(const bdpt_sphere* sp, unsigned n, bool zero_exit_safe) {
    bdpt_jit_scene s;
    s.n = n;
    s.zero_exit = zero_exit_safe;
    s.geom = "{";
    for (unsigned i = 0; i < n; i++) {
        const bdpt_vec& e = sp[i].e;
        if (!(e.x == 0.f && e.y == 0.f && e.z == 0.f)) {
            if (i < 64) s.emis |= 1ull << i;
        } else {
            s.n_vac++;
        }
        const float rr = sp[i].rad * sp[i].rad;              // the product the scene upload forms
        s.geom += (i ? ",{" : "{") + bdpt_jit_hexf(sp[i].p.x) + "," + bdpt_jit_hexf(sp[i].p.y) + "," +
                  bdpt_jit_hexf(sp[i].p.z) + "," + bdpt_jit_hexf(rr) + "}";
    }
    s.geom += "}";
    return s;
}

// One build of a variant: the waves/SIMD it targets, the 2-KB sincos table of even entries
// (bdpt_math.h) in place of the 4-KB one, and the lane-group loop in place of the straight-line
// part-full shadow rounds.
struct bdpt_jit_attempt {
    int waves = 0;
    bool coarse = false, pf_off = false;
    bool operator==(const bdpt_jit_attempt& o) const { return waves == o.waves && coarse == o.coarse && pf_off == o.pf_off; }
};

// Waves/SIMD the first build targets: 6 for the pass-stream kernels, 5 for the fused S = 1 kernel
// (at 6 it fits without spills, but then the LDS estimate of bdpt_jit_judge takes the 2-KB sincos
// table and caustic8 measured 0.6 % slower than 5 waves with the 4-KB table), or the override.
inline bdpt_jit_attempt bdpt_jit_first_attempt(const bdpt_jit_variant& v, const bdpt_jit_env& env) {
    bdpt_jit_attempt a;
    a.waves = v.streams() ? (env.has_waves ? env.waves : 6) : (env.has_fused_waves ? env.fused_waves : 5);
    return a;
}

// The name expression of the instance (a launch over a tile list runs the instance with the
// tile-list code; -DBDPT_TILES=1 gives the kernel that name).
inline std::string bdpt_jit_name(const bdpt_jit_variant& v, const bdpt_jit_scene& s) {
    return std::string(v.tiles ? "&bdpt_path_tiles_kernel_t<" : "&bdpt_path_kernel_t<") + std::to_string(s.n) +
           (v.streams() ? ", true>" : ", false>");
}

// The compile options of an attempt.  With the name they key the per-context table of builds and
// the on-disk cache, so neither a string nor the order may change without renaming every cached
// code object.
inline std::vector<std::string> bdpt_jit_options(const bdpt_jit_variant& v, const bdpt_jit_scene& s,
                                                 const bdpt_jit_env& env, const bdpt_jit_attempt& a) {
    std::vector<std::string> o = {
        "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize",
        "-fno-gpu-flush-denormals-to-zero", "-DBDPT_JIT=1", "-DBDPT_JIT_N=" + std::to_string(s.n),
        "-DBDPT_JIT_EMIS=" + std::to_string(s.emis) + "ull", "-DBDPT_JIT_GEOM=" + s.geom,
        "-DBDPT_JIT_ZERO_SAFE=" + std::to_string(s.zero_exit ? 1 : 0),
        "-DBDPT_WAVES_PER_SIMD=" + std::to_string(a.waves)};
    if (!v.streams()) o.push_back("-DBDPT_FUSED_WAVES=" + std::to_string(a.waves));
    if (!v.streams() && !v.pair) o.push_back("-DBDPT_RNG_PAIR=0");
    if (v.pool()) o.push_back("-DBDPT_POOL=1");
    if (v.units()) o.push_back("-DBDPT_UNITS=1");
    if (v.tiles) o.push_back("-DBDPT_TILES=1");
    if (!s.vac_list()) o.push_back("-DBDPT_VAC_LIST=0");
    // Part-full shadow rounds as straight-line code (BDPT_PF_UNROLL of the kernel source, on by
    // default in these builds; the user's flags set it either way): not in the pixel-pool build,
    // which has not been measured with it, and not where the build with it spills at more than 5
    // waves/SIMD (pf_off: the bodies change the register allocation of the whole loop, and the
    // in-kernel fold build of synthetic64 then needs scratch at 6)
    if (!env.pf_user() && (v.pool() || a.pf_off)) o.push_back("-DBDPT_PF_UNROLL=0");
    for (std::string& t : env.tokens()) o.push_back(std::move(t));
    if (a.coarse) o.push_back("-DBDPT_SC_COARSE=1");
    return o;
}

struct bdpt_jit_verdict {
    bool keep;                       // run this build; else build `next`
    bdpt_jit_attempt next;
};

// What to do with the build of attempt `a`, given what the loaded function reports:
// static_lds_bytes, its static LDS, or -1 when that query failed (the coarse-table test is then
// skipped), and scratch_bytes, its scratch per lane, 0 when that query failed (a build whose
// spills cannot be read counts as spill-free).
//  1. The 4-KB sincos table costs a workgroup per CU when LDS bounds the count (large scenes: 16 B
//     per sphere; the fused kernel: a VLP and a sid per pass of the launch): then the same waves
//     with the 2-KB table.  Estimated with the launches' LDS formula (bdpt_plan.h) over a table of
//     5 per sphere and the pass slots of the kind: one for the pass-stream kernel, a range of
//     passes for the units, fused_max_passes for the fused.  Not when the user's flags name the table.
//  2. A build that spills above the 5-wave floor is tried once more at the same waves with the
//     lane-group loop in place of the straight-line part-full rounds (not the pool build, which
//     never has them, nor when the user's flags name them).
//  3. Spill-free, at or below the floor, or BDPT_JIT_SCRATCH_OK: kept.  Else one wave less.
inline bdpt_jit_verdict bdpt_jit_judge(const bdpt_jit_variant& v, const bdpt_jit_scene& s, const bdpt_jit_env& env,
                                       const bdpt_jit_attempt& a, int static_lds_bytes, int scratch_bytes) {
    bdpt_jit_attempt next = a;
    if (!a.coarse && !env.user_coarse() && static_lds_bytes >= 0) {
        const size_t slots = v.units() ? (size_t)std::max(env.units, 16) : v.streams() ? 1 : (size_t)env.fused_max_passes;
        const size_t dyn = bdpt_path_smem(5 * (size_t)s.n, slots, 0, 0), stat = (size_t)static_lds_bytes;
        const size_t lds = 160 * 1024, fine = lds / (dyn + stat), half = lds / (dyn + stat - 2048);
        if (fine < (size_t)a.waves && half > fine) {
            next.coarse = true;
            return {false, next};
        }
    }
    if (scratch_bytes != 0 && a.waves > 5 && !a.pf_off && !env.pf_user() && !v.pool() && !env.scratch_ok) {
        next.pf_off = true;
        return {false, next};
    }
    if (scratch_bytes == 0 || a.waves <= 5 || env.scratch_ok) return {true, a};
    next.waves = a.waves - 1;
    return {false, next};
}

#endif
