// bdpt_filter.h -- the per-pixel and per-tap arithmetic of the frame services (include/bdpt.h:
// bdpt_denoise, bdpt_preview_denoise, bdpt_denoise_noise, bdpt_reproject, bdpt_noise_estimate),
// stated once for both backends.  Two drivers run it: the HIP kernels (bdpt_frame_kernels.h: tiles,
// LDS staging, the wave reduction) and the CPU backend (bdpt_cpu.cpp: rows over threads).  The
// numpy models in tests/*_common.py are the independent statement both are checked against.
//
// Numerics: the definitions in include/bdpt.h operation for operation -- fp32, no contraction
// (-ffp-contract=off), dot() as (x*x' + y*y') + z*z', every reciprocal, division and root correctly
// rounded, denormals kept.  A tap that is not used adds nothing: it is skipped, not weighted by 0.
//
// What a translation unit brings with it (f3 and its operations, the constants, the reciprocals
// and the root) is bdpt_sides.h's, the one block with two definitions.
#pragma once
#include "bdpt_sides.h"

namespace {

// ---------------------------------------------------------------------------------------------
// Small constants and rules

// the 5 x 5 B3-spline weight of tap (j, t): h[j] * h[t], an exact constant
BDPT_BOTH float b3_weight(int j, int t) {
    constexpr float hk[5] = {1.f / 16.f, 1.f / 4.f, 3.f / 8.f, 1.f / 4.f, 1.f / 16.f};
    return hk[j] * hk[t];
}

// The guide id of a pixel: the first hit's sphere, or -1 where the pixel is not to be filtered (a
// miss; unless all_materials, any sphere that is not DIFF).  Eligibility is a function of the
// sphere, so "same sphere as an eligible centre" implies an eligible tap.
template <class Sphere>
BDPT_BOTH int guide_id(int id, bool all_materials, const Sphere* sph) {
    int g = id;
    if (g >= 0 && !all_materials && sph[g].refl != kFltDiff) g = -1;
    return g;
}
// The guide key of a pixel whose unjittered TRANSMIT chain ends on a diffuse surface (include/bdpt.h
// BDPT_DENOISE_THROUGH; -1: it does not): the end sphere itself after no bounce, else a key of the
// bounce count, the first sphere and the end sphere, above the n sphere ids.  The caller has checked
// that 6 n^2 + n fits an int.
BDPT_BOTH int through_key(bool diffuse, int n, int bounces, int first_id, int id) {
    if (!diffuse) return -1;
    return bounces == 0 ? id : n + ((bounces - 1) * n + first_id) * n + id;
}

// clampc of bdpt_preview_denoise: a record's count, 0 or inside [2^-20, 2^40]
BDPT_BOTH float clampc(float w) { return w == 0.f ? 0.f : fminf(fmaxf(w, 0x1p-20f), 0x1p40f); }

// ---------------------------------------------------------------------------------------------
// The a-trous level of the three filters: taps and finishes.  What a pixel carries next to its
// colour through the levels: nothing (bdpt_denoise), the sample count (bdpt_preview_denoise) or the
// variance (bdpt_denoise_noise).
constexpr int kLvPlain = 0, kLvCounts = 1, kLvNoise = 2;

// the normal weight of a tap: the cosine, clamped at 0, squared np = normal_power times
BDPT_BOTH float tap_wn(f3 n_p, f3 n_q, int np) {
    const float d = dot(n_p, n_q);
    float wn = d > 0.f ? d : 0.f;
    for (int r = 0; r < np; r++) wn = wn * wn;
    return wn;
}

BDPT_BOTH float tap_e2(f3 c_p, f3 q) {
    const f3 dc = sub(q, c_p);
    return dot(dc, dc);
}

// one used tap of bdpt_denoise: hw = b3_weight(j, t), q the tap's colour
BDPT_BOTH void dn_tap(float hw, int np, float isc, f3 n_p, f3 c_p, f3 n_q, f3 q, float& sw, f3& sc) {
    const float wn = tap_wn(n_p, n_q, np);
    const float e2 = tap_e2(c_p, q);
    const float wc = flt_rcp_ge1(1.f + e2 * isc);        // e2 >= 0 and isc >= 0, or their product is NaN
    const float w = (hw * wn) * wc;
    sw = sw + w;
    sc = add(sc, smul(w, q));
}

// one used tap with counts (a_q > 0); a centre without a count (a_p == 0) stops nothing: wc = 1.f.
// a_p + a_q lies in [2^-20, 2^41] (clampc), inside the fast reciprocal's range
BDPT_BOTH void pv_tap(float hw, int np, float isc, float c2, f3 n_p, f3 c_p, float a_p, f3 n_q, f3 q, float a_q,
                     float& su, float& sw, f3& sc) {
    const float wn = tap_wn(n_p, n_q, np);
    const float e2 = tap_e2(c_p, q);
    float wc = 1.f;
    if (a_p != 0.f) {
        const float g = ((a_p * a_q) * flt_rcp_inrange(a_p + a_q)) * c2;
        wc = flt_rcp_ge1(1.f + (e2 * isc) * g);          // the product is non-negative or NaN
    }
    const float u = (hw * wn) * wc;
    const float w = u * a_q;
    su = su + u;
    sw = sw + w;
    sc = add(sc, smul(w, q));
}

// one used tap of bdpt_denoise_noise: the colour stop from the two variances where both pixels
// have one (v < 0: none), else the denoiser's; the centre's variance is carried as sum w^2 v
BDPT_BOTH void nz_tap(float hw, int np, float isc, float s2, f3 n_p, f3 c_p, float v_p, f3 n_q, f3 q, float v_q,
                     float& sv, float& sw, f3& sc) {
    const float wn = tap_wn(n_p, n_q, np);
    const float e2 = tap_e2(c_p, q);
    const bool has_p = !(v_p < 0.f), has_q = !(v_q < 0.f);
    float wc;
    if (has_p && has_q) {
        const float t = s2 * (v_p + v_q) + kFltNoiseEps;
        wc = t * flt_rcp(t + e2);
    } else {
        wc = flt_rcp_ge1(1.f + e2 * isc);
    }
    const float w = (hw * wn) * wc;
    sw = sw + w;
    sc = add(sc, smul(w, q));
    if (has_p) sv = sv + (w * w) * (has_q ? v_q : v_p);
}

// One tap that is inside the frame and shows the centre's sphere.  a_p, a_q: the centre's and the
// tap's count or variance; k: c2 = 2 / count_ref (counts) or s2 = noise_sigma^2 (noise); su: the
// second sum (counts: of u; noise: of w^2 v); used (counts): the tap had a count.
template <int MODE>
BDPT_BOTH void lv_tap(float hw, int np, float isc, float k, f3 n_p, f3 c_p, float a_p, f3 n_q, f3 q, float a_q,
                     float& su, float& sw, f3& sc, bool& used) {
    if constexpr (MODE == kLvCounts) {
        if (!(a_q > 0.f)) return;
        pv_tap(hw, np, isc, k, n_p, c_p, a_p, n_q, q, a_q, su, sw, sc);
        used = true;
    } else if constexpr (MODE == kLvNoise) {
        nz_tap(hw, np, isc, k, n_p, c_p, a_p, n_q, q, a_q, su, sw, sc);
    } else {
        dn_tap(hw, np, isc, n_p, c_p, n_q, q, sw, sc);
    }
}

// The centre's colour from the sums, and in `a` what it carries on.  Counts: with no tap counted
// the centre is copied through, else the count is clampc(sw / su).  Noise: the variance of the
// weighted mean, (sum w^2 v) / (sum w)^2 as (su * r) * r, where the centre had one.
template <int MODE>
BDPT_BOTH f3 lv_finish(bool used, f3 c_p, float a_p, float su, float sw, f3 sc, float& a) {
    if constexpr (MODE == kLvCounts) {
        if (!used) {
            a = a_p;
            return c_p;
        }
        a = clampc(sw / su);
        return smul(flt_rcp(sw), sc);
    } else if constexpr (MODE == kLvNoise) {
        const float r = flt_rcp(sw);
        const f3 o = smul(r, sc);
        a = !(a_p < 0.f) ? (su * r) * r : a_p;
        return o;
    } else {
        a = 0.f;
        return smul(flt_rcp(sw), sc);
    }
}

// ---------------------------------------------------------------------------------------------
// The variance prefilter of bdpt_denoise_noise: one tap inside the frame (used where it shows the
// centre's sphere and has a variance), and the centre's result
BDPT_BOTH void pf_tap(float hw, bool same_sphere, float v_q, float& sv, float& sh, bool& used) {
    if (!same_sphere || v_q < 0.f) return;
    sv = sv + hw * v_q;
    sh = sh + hw;
    used = true;
}
BDPT_BOTH float pf_finish(bool used, float sv, float sh) { return used ? sv / sh : -1.0f; }

// ---------------------------------------------------------------------------------------------
// The mark of bdpt_noise_estimate: a pixel's colour A at count mn, against its colour B at cnt now

// the mark is usable: mn > 0, cnt > mn and 2 * (cnt - mn) >= mn, the last as
// cnt - mn >= ceil(mn / 2) so that 32 bits cannot wrap
BDPT_BOTH bool mark_valid(unsigned cnt, unsigned mn) {
    return mn > 0u && cnt > mn && cnt - mn >= (mn >> 1) + (mn & 1u);
}
BDPT_BOTH bool mark_growing(unsigned cnt) { return cnt > 0u && cnt < kFltCounterCap; }
// a re-marking call takes the pixel: it still grows and cnt >= 2 * mn, as (cnt >> 1) >= mn
BDPT_BOTH bool mark_take(unsigned cnt, unsigned mn) { return mark_growing(cnt) && (cnt >> 1) >= mn; }

// the raw variance v0 of a pixel with a valid mark (bdpt_denoise_noise)
BDPT_BOTH float raw_variance(f3 B, f3 A, unsigned cnt, unsigned mn) {
    const f3 d = sub(B, A);
    const float a = (float)mn, n = (float)cnt;
    return dot(d, d) * (a / (n - a));
}

// the per-pixel error of a pixel with a valid mark (bdpt_noise_estimate)
BDPT_BOTH float pixel_error(f3 B, f3 A, unsigned cnt, unsigned mn, float dark) {
    const float a = (float)mn, n = (float)cnt;
    const float dx = B.x - A.x, dy = B.y - A.y, dz = B.z - A.z;
    const float e1 = (fabsf(dx) + fabsf(dy)) + fabsf(dz);
    const float s = a / (n - a);
    const float f = flt_sqrt(s);
    const float lum = (B.x + B.y) + B.z;
    const float den = flt_sqrt(fmaxf(lum, dark));
    return (e1 * f) / den;
}

// ---------------------------------------------------------------------------------------------
// Temporal reprojection (bdpt_reproject)

// The first-hit point P in the history's camera (origin o, unit axes ux, uy, ud; hw, hh the film's
// half extent, sx, sy pixels per film unit): its continuous pixel position, and whether the four
// taps around it can touch the frame (a NaN fails).  cz = 0 takes the library division.
BDPT_BOTH bool rp_project(f3 P, f3 o, f3 ux, f3 uy, f3 ud, float hw, float hh, float sx, float sy, int W, int H,
                         float& fx, float& fy) {
    const f3 d = sub(P, o);
    const float a = dot(d, ux);
    const float b = dot(d, uy);
    const float cz = dot(d, ud);
    const float r = flt_rcp(cz);
    const float kx = (10.f * a) * r, ky = (10.f * b) * r;
    fx = (kx + hw) * sx;
    fy = (ky + hh) * sy;
    return fx >= -1.f && fx < (float)W && fy >= -1.f && fy < (float)H;
}

// "Follow" (bdpt_history_follow): the first-hit point where its sphere was when the history was
// taken, P' = P - delta[id1].  It replaces P in rp_project and in rp_tap's plane test and nowhere
// else.  x - (+0) == x for every x, -0 included, so an unmoved sphere's pixel keeps P's bits.
BDPT_BOTH f3 rp_follow(f3 P, f3 delta) { return sub(P, delta); }

// Bilinear tap k (dx = k & 1, dy = k >> 1; dy outer, dx inner, as defined) with the fractions
// (wx, wy).  in: the tap is inside the frame; where it is not, the caller passes any record.  The
// tap counts where its weight is positive, it shows the pixel's sphere id1, has a count m_q > 0
// and its point p_q lies within lim of the plane (P, N).
BDPT_BOTH void rp_tap(int k, float wx, float wy, bool in, int id_q, f3 p_q, f3 c_q, float m_q, int id1, f3 P, f3 N,
                     float lim, float max_history, float& sw, float& sm, f3& sc, bool& used) {
    const float bx = (k & 1) ? wx : 1.f - wx, by = (k >> 1) ? wy : 1.f - wy;
    const float bw = bx * by;
    if (!in || !(bw > 0.f) || id_q != id1 || !(m_q > 0.f)) return;
    if (!(fabsf(dot(sub(p_q, P), N)) <= lim)) return;
    sw = sw + bw;
    sm = sm + bw * fminf(m_q, max_history);
    sc = add(sc, smul(bw, c_q));
    used = true;
}

// the history (h, m) from the taps' sums; a denormal sw takes the library division
BDPT_BOTH void rp_history(bool used, float sw, float sm, f3 sc, f3& h, float& m) {
    if (used) {
        h = smul(flt_rcp(sw), sc);
        m = sm;
    }
}

// the blend of the frame's (c, n) with the history's (h, m); tot = n + m
BDPT_BOTH f3 rp_blend(f3 c, float n, f3 h, float m, float& tot) {
    tot = n + m;
    f3 o = c;
    if (m == 0.f) {
    } else if (n == 0.f) {
        o = h;
    } else {
        const float rt = flt_rcp(tot);
        o = mk((n * c.x + m * h.x) * rt, (n * c.y + m * h.y) * rt, (n * c.z + m * h.z) * rt);
    }
    return o;
}

}  // namespace

#undef BDPT_BOTH
