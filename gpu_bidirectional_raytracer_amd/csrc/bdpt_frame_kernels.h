// bdpt_frame_kernels.h -- the kernels of the frame services (bdpt_frame.cpp): denoiser, temporal
// reprojection, denoised preview and noise estimate.  Part of bdpt_kernels.hip, which includes this
// file in its precompiled build only (never under BDPT_JIT), after the helpers used here: f3 and
// its operations, rcp_rn, bdpt_sqrt_rn, bdpt_dev_to_rgba.  bdpt_aov_kernel, whose planes these
// kernels read, stays there with the path kernel's traversal.

// ---------------------------------------------------------------------------------------------
// Edge-avoiding wavelet denoiser (include/bdpt.h bdpt_denoise; no reference
// counterpart).  Host sequence on the context's stream: bdpt_aov_kernel (unjittered, whole frame),
// bdpt_denoise_pack_kernel, then one level kernel per level, ping-pong.
//
// Numerics: the definition in include/bdpt.h, operation for operation -- fp32, no contraction
// (-ffp-contract=off), dot() in the order (x + y) + z, both divisions correctly rounded (rcp_rn:
// v_rcp_f32 + one Newton step inside [2^-125, 2^125), the library division outside, e.g. for
// 1 + e2 * isc = +inf).  Denormal intermediates are kept, not flushed: wn (a cosine squared up to
// six times) and w underflow gradually, and the build keeps fp32 denormals (hipcc's default for
// gfx9; the hipRTC flags of the specialised kernels say -fno-gpu-flush-denormals-to-zero
// explicitly).  A tap that is not used adds nothing -- it is skipped, not weighted by zero.

// Guide records and the first ping buffer.  gid: the first hit's sphere, or -1 where the pixel is
// not to be filtered (a miss; with materials == DIFFUSE any sphere that is not DIFF).  Eligibility
// is a function of the sphere, so "same sphere as an eligible centre" implies an eligible tap.
extern "C" __global__ __launch_bounds__(256) void bdpt_denoise_pack_kernel(
    const int* __restrict__ id, const bdpt_dev_vec* __restrict__ normal, const bdpt_dev_vec* __restrict__ colors,
    const bdpt_dev_sphere* __restrict__ sph, int all_materials, float4* __restrict__ guide,
    float4* __restrict__ ping, int count) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    int g = id[i];
    if (g >= 0 && !all_materials && sph[g].refl != BDPT_DEV_DIFF) g = -1;
    const bdpt_dev_vec n = normal[i];
    guide[i] = make_float4(n.x, n.y, n.z, __int_as_float(g));
    if (ping) {                                          // nullptr: the guide records alone
        const bdpt_dev_vec c = colors[i];
        ping[i] = make_float4(c.x, c.y, c.z, 0.f);
    }
}

// 1.f / x, correctly rounded, for x >= 1 or NaN (1 + a product that is non-negative or NaN): one
// compare decides between the in-range sequence and the library division (+inf, NaN, >= 2^125)
__device__ __forceinline__ float rcp_rn_ge1(float x) {
    if (__builtin_expect(!(x < 0x1p125f), 0)) return 1.f / x;
    return rcp_rn_inrange(x);
}

// clampc of bdpt_preview_denoise: a record's count, 0 or inside [2^-20, 2^40]
__device__ __forceinline__ float pv_clampc(float w) { return w == 0.f ? 0.f : fminf(fmaxf(w, 0x1p-20f), 0x1p40f); }

// The level kernels of both filters.  bdpt_preview_denoise (include/bdpt.h) runs
// bdpt_aov_kernel once, bdpt_reproject_kernel writing its {o, clampc(tot)} record into the ping
// buffer and the guide record next to it, then one level per level as the denoiser does: its level
// kernels are the denoiser's with the count in the colour record's .w (kLvCounts below) -- the same
// 32-byte records, tiles and LDS staging.  Numerics as above; a_p + a_q lies in [2^-20, 2^41],
// inside the fast reciprocal's range, and sw / su is the library division.

// one used tap: hw = h[j] * h[i] (an exact constant), NP squarings of the normal weight
template <int NP>
__device__ __forceinline__ void dn_tap(float hw, float isc, f3 n_p, f3 c_p, float4 gq, float4 cq, float& sw, f3& sc) {
    const float d = dot(n_p, mk(gq.x, gq.y, gq.z));
    float wn = d > 0.f ? d : 0.f;
#pragma unroll
    for (int r = 0; r < NP; r++) wn = wn * wn;
    const f3 q = mk(cq.x, cq.y, cq.z);
    const f3 dc = sub(q, c_p);
    const float e2 = dot(dc, dc);
    const float wc = rcp_rn_ge1(1.f + e2 * isc);        // e2 >= 0 and isc >= 0, or their product is NaN
    const float w = (hw * wn) * wc;
    sw = sw + w;
    sc = add(sc, smul(w, q));
}

// one used tap with counts (a_q > 0); a centre without a count (a_p == 0) stops nothing: wc = 1.f
template <int NP>
__device__ __forceinline__ void pv_tap(float hw, float isc, float c2, f3 n_p, f3 c_p, float a_p, float4 gq, float4 cq,
                                       float& su, float& sw, f3& sc) {
    const float d = dot(n_p, mk(gq.x, gq.y, gq.z));
    float wn = d > 0.f ? d : 0.f;
#pragma unroll
    for (int r = 0; r < NP; r++) wn = wn * wn;
    const f3 q = mk(cq.x, cq.y, cq.z);
    const f3 dc = sub(q, c_p);
    const float e2 = dot(dc, dc);
    const float a_q = cq.w;
    float wc = 1.f;
    if (a_p != 0.f) {
        const float g = ((a_p * a_q) * rcp_rn_inrange(a_p + a_q)) * c2;
        wc = rcp_rn_ge1(1.f + (e2 * isc) * g);           // the product is non-negative or NaN
    }
    const float u = (hw * wn) * wc;
    const float w = u * a_q;
    su = su + u;
    sw = sw + w;
    sc = add(sc, smul(w, q));
}

// one used tap of bdpt_denoise_noise (include/bdpt.h): the colour stop from the two
// variances where both pixels have one (v < 0: none), else the denoiser's; the centre's variance is
// carried as sum w^2 v
template <int NP>
__device__ __forceinline__ void nz_tap(float hw, float isc, float s2, f3 n_p, f3 c_p, float v_p, float4 gq, float4 cq,
                                       float& sv, float& sw, f3& sc) {
    const float d = dot(n_p, mk(gq.x, gq.y, gq.z));
    float wn = d > 0.f ? d : 0.f;
#pragma unroll
    for (int r = 0; r < NP; r++) wn = wn * wn;
    const f3 q = mk(cq.x, cq.y, cq.z);
    const f3 dc = sub(q, c_p);
    const float e2 = dot(dc, dc);
    const float v_q = cq.w;
    const bool has_p = !(v_p < 0.f), has_q = !(v_q < 0.f);
    float wc;
    if (has_p && has_q) {
        const float t = s2 * (v_p + v_q) + BDPT_DEV_DNOISE_EPS;
        wc = t * rcp_rn(t + e2);
    } else {
        wc = rcp_rn_ge1(1.f + e2 * isc);
    }
    const float w = (hw * wn) * wc;
    sw = sw + w;
    sc = add(sc, smul(w, q));
    if (has_p) sv = sv + (w * w) * (has_q ? v_q : v_p);
}

// What the colour record's .w carries through the levels: nothing (bdpt_denoise), the sample count
// (bdpt_preview_denoise) or the variance (bdpt_denoise_noise).
constexpr int kLvPlain = 0, kLvCounts = 1, kLvNoise = 2;

// One pixel's result: the next buffer's record (with the count or the variance a; plain: .w = 0)
// and the packed results the last level was asked for.
template <int MODE, class Args>
__device__ __forceinline__ void level_store(const Args& v, int i, f3 o, float a) {
    if (v.nxt) v.nxt[i] = make_float4(o.x, o.y, o.z, MODE != kLvPlain ? a : 0.f);
    if (v.out3) {
        bdpt_dev_vec ov;
        ov.x = o.x; ov.y = o.y; ov.z = o.z;
        v.out3[i] = ov;
    }
    if constexpr (MODE == kLvCounts) {
        if (v.weight) v.weight[i] = a;
    }
    if constexpr (MODE == kLvNoise) {
        if (v.variance) v.variance[i] = a;
    }
    if (v.rgba) v.rgba[i] = bdpt_dev_to_rgba(o.x, o.y, o.z, v.gamma_thr);
}

// one tap that passed the id test; counts: used only where the tap has a count.  su: the second sum
// (counts: of u; noise: of w^2 v)
template <int NP, int MODE, class Args>
__device__ __forceinline__ void level_tap(const Args& v, float hw, f3 n_p, f3 c_p, float a_p, float4 gq, float4 cq,
                                          float& su, float& sw, f3& sc, bool& used) {
    if constexpr (MODE == kLvCounts) {
        if (!(cq.w > 0.f)) return;
        pv_tap<NP>(hw, v.isc, v.c2, n_p, c_p, a_p, gq, cq, su, sw, sc);
        used = true;
    } else if constexpr (MODE == kLvNoise) {
        nz_tap<NP>(hw, v.isc, v.s2, n_p, c_p, a_p, gq, cq, su, sw, sc);
    } else {
        dn_tap<NP>(hw, v.isc, n_p, c_p, gq, cq, sw, sc);
    }
}

// the centre's result from the sums; `used` (counts): at least one tap counted, else the centre is
// copied through; noise: the variance of the weighted mean, (sum w^2 v) / (sum w)^2, where the
// centre had one
template <int MODE, class Args>
__device__ __forceinline__ void level_finish(const Args& v, int i, bool used, f3 c_p, float a_p, float su, float sw,
                                             f3 sc) {
    if constexpr (MODE == kLvCounts) {
        if (!used) {
            level_store<MODE>(v, i, c_p, a_p);
            return;
        }
        level_store<MODE>(v, i, smul(rcp_rn(sw), sc), pv_clampc(sw / su));
    } else if constexpr (MODE == kLvNoise) {
        const float r = rcp_rn(sw);
        level_store<MODE>(v, i, smul(r, sc), !(a_p < 0.f) ? (su * r) * r : a_p);
    } else {
        level_store<MODE>(v, i, smul(rcp_rn(sw), sc), 0.f);
    }
}

// One level, taps straight from L1 / L2: one lane per pixel, two 16-byte loads per tap (guide
// record and colour), one 16-byte store.  Wave tiles 8 x 8 or 64 x 1
// (v.rows), as in bdpt_aov_kernel.  The 25 taps are unrolled, j outer and i inner as defined.
template <int NP, int MODE, class Args>
__device__ __forceinline__ void level_direct(const Args& v) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = v.rows ? (int)blockIdx.x * BDPT_DN_ROW_BTW + lane
                         : (int)blockIdx.x * BDPT_DN_BTW + wave * 8 + (lane & 7);
    const int y = v.rows ? (int)blockIdx.y * BDPT_DN_ROW_BTH + wave
                         : (int)blockIdx.y * BDPT_DN_BTH + (lane >> 3);
    if (x >= v.W || y >= v.H) return;                    // (no cross-lane operation below)
    const int i = y * v.W + x;
    const float4 gp = v.guide[i], cp4 = v.cur[i];
    const f3 c_p = mk(cp4.x, cp4.y, cp4.z);
    const float a_p = cp4.w;                             // the centre's count or variance
    const int gid = __float_as_int(gp.w);
    if (gid < 0) {                                       // copied through, colour and .w
        level_store<MODE>(v, i, c_p, a_p);
        return;
    }
    const f3 n_p = mk(gp.x, gp.y, gp.z);
    constexpr float hk[5] = {1.f / 16.f, 1.f / 4.f, 3.f / 8.f, 1.f / 4.f, 1.f / 16.f};
    float su = 0.f, sw = 0.f;
    f3 sc = mk(0.f, 0.f, 0.f);
    bool used = false;
#pragma unroll
    for (int j = 0; j < 5; j++) {
        const int qy = y + (j - 2) * v.step;
        if (qy < 0 || qy >= v.H) continue;
        // the row's ten loads are issued together; a tap outside the frame reads the centre
        // (always a valid address) and is not used
        float4 gq[5], cq[5];
        bool in[5];
#pragma unroll
        for (int t = 0; t < 5; t++) {
            const int qx = x + (t - 2) * v.step;
            in[t] = qx >= 0 && qx < v.W;
            const int q = in[t] ? qy * v.W + qx : i;
            gq[t] = v.guide[q];
            cq[t] = v.cur[q];
        }
#pragma unroll
        for (int t = 0; t < 5; t++)
            if (in[t] && __float_as_int(gq[t].w) == gid)
                level_tap<NP, MODE>(v, hk[j] * hk[t], n_p, c_p, a_p, gq[t], cq[t], su, sw, sc, used);
    }
    level_finish<MODE>(v, i, used, c_p, a_p, su, sw, sc);
}

// The same level with the 32 x 8 tile and its halo of 2 * step <= 4 pixels staged in LDS (steps 1
// and 2, where neighbouring lanes share most taps): every record of the region is loaded from
// memory once per workgroup, coalesced, and the 25 taps are ds reads.  Positions outside the
// frame hold the id -2, which no eligible centre has.  Kept or not by measurement: DESIGN.md 4d.
template <int NP, int MODE, class Args>
__device__ __forceinline__ void level_staged(const Args& v) {
    __shared__ float4 sg[BDPT_DN_LDS_W * BDPT_DN_LDS_H], scol[BDPT_DN_LDS_W * BDPT_DN_LDS_H];
    const int halo = 2 * v.step;                         // <= 4 (the host launches steps 1 and 2 only)
    const int rw = BDPT_DN_BTW + 2 * halo, rh = BDPT_DN_BTH + 2 * halo;
    const int bx0 = (int)blockIdx.x * BDPT_DN_BTW - halo, by0 = (int)blockIdx.y * BDPT_DN_BTH - halo;
    for (int k = threadIdx.x; k < rw * rh; k += 256) {   // rw * rh <= BDPT_DN_LDS_W * BDPT_DN_LDS_H
        const int ry = k / rw, rx = k - ry * rw;
        const int gx = bx0 + rx, gy = by0 + ry;
        float4 g = make_float4(0.f, 0.f, 0.f, __int_as_float(-2)), c = make_float4(0.f, 0.f, 0.f, 0.f);
        if (gx >= 0 && gx < v.W && gy >= 0 && gy < v.H) {
            g = v.guide[gy * v.W + gx];
            c = v.cur[gy * v.W + gx];
        }
        sg[k] = g;
        scol[k] = c;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lx = wave * 8 + (lane & 7), ly = lane >> 3;
    const int x = (int)blockIdx.x * BDPT_DN_BTW + lx, y = (int)blockIdx.y * BDPT_DN_BTH + ly;
    if (x >= v.W || y >= v.H) return;
    const int i = y * v.W + x, li = (ly + halo) * rw + lx + halo;
    const float4 gp = sg[li], cp4 = scol[li];
    const f3 c_p = mk(cp4.x, cp4.y, cp4.z);
    const float a_p = cp4.w;
    const int gid = __float_as_int(gp.w);
    if (gid < 0) {
        level_store<MODE>(v, i, c_p, a_p);
        return;
    }
    const f3 n_p = mk(gp.x, gp.y, gp.z);
    constexpr float hk[5] = {1.f / 16.f, 1.f / 4.f, 3.f / 8.f, 1.f / 4.f, 1.f / 16.f};
    float su = 0.f, sw = 0.f;
    f3 sc = mk(0.f, 0.f, 0.f);
    bool used = false;
#pragma unroll
    for (int j = 0; j < 5; j++) {
#pragma unroll
        for (int t = 0; t < 5; t++) {
            const int q = li + (j - 2) * v.step * rw + (t - 2) * v.step;
            const float4 gq = sg[q];
            if (__float_as_int(gq.w) != gid) continue;
            level_tap<NP, MODE>(v, hk[j] * hk[t], n_p, c_p, a_p, gq, scol[q], su, sw, sc, used);
        }
    }
    level_finish<MODE>(v, i, used, c_p, a_p, su, sw, sc);
}

template <int NP>
__global__ __launch_bounds__(256) void bdpt_denoise_level_t(bdpt_denoise_args v) { level_direct<NP, kLvPlain>(v); }
template <int NP>
__global__ __launch_bounds__(256) void bdpt_denoise_level_lds_t(bdpt_denoise_args v) { level_staged<NP, kLvPlain>(v); }
template <int NP>
__global__ __launch_bounds__(256) void bdpt_preview_level_t(bdpt_preview_args v) { level_direct<NP, kLvCounts>(v); }
template <int NP>
__global__ __launch_bounds__(256) void bdpt_preview_level_lds_t(bdpt_preview_args v) { level_staged<NP, kLvCounts>(v); }
template <int NP>
__global__ __launch_bounds__(256) void bdpt_dnoise_level_t(bdpt_dnoise_args v) { level_direct<NP, kLvNoise>(v); }
template <int NP>
__global__ __launch_bounds__(256) void bdpt_dnoise_level_lds_t(bdpt_dnoise_args v) { level_staged<NP, kLvNoise>(v); }

// host-side launch tables: [LDS staging][normal_power]
#define BDPT_LEVEL_ROW(K) \
    {(const void*)&K<0>, (const void*)&K<1>, (const void*)&K<2>, (const void*)&K<3>, (const void*)&K<4>, \
     (const void*)&K<5>, (const void*)&K<6>}
extern "C" const void* bdpt_denoise_level_table[2][7] = {BDPT_LEVEL_ROW(bdpt_denoise_level_t),
                                                         BDPT_LEVEL_ROW(bdpt_denoise_level_lds_t)};
extern "C" const void* bdpt_preview_level_table[2][7] = {BDPT_LEVEL_ROW(bdpt_preview_level_t),
                                                         BDPT_LEVEL_ROW(bdpt_preview_level_lds_t)};
extern "C" const void* bdpt_dnoise_level_table[2][7] = {BDPT_LEVEL_ROW(bdpt_dnoise_level_t),
                                                        BDPT_LEVEL_ROW(bdpt_dnoise_level_lds_t)};
#undef BDPT_LEVEL_ROW

// ---------------------------------------------------------------------------------------------
// The noise-guided denoiser's own kernels (include/bdpt.h bdpt_denoise_noise; no
// reference counterpart).  Host sequence on the context's stream: bdpt_aov_kernel,
// bdpt_dnoise_pack_kernel, bdpt_dnoise_prefilter_kernel, then the bdpt_dnoise_level_t instances
// above, ping-pong from the prefilter's output.  Numerics as for the denoiser; a / (n - a) and
// sv / sh are the compiler's correctly rounded divisions (denormals kept).

// Guide records as bdpt_denoise_pack_kernel writes them, and {B, raw variance v0 or -1} into the
// ping buffer.  mark: the noise estimate's records, nullptr while none was ever stored; live = 0:
// the mark is cleared (every count reads 0).
extern "C" __global__ __launch_bounds__(256) void bdpt_dnoise_pack_kernel(
    const int* __restrict__ id, const bdpt_dev_vec* __restrict__ normal, const bdpt_dev_vec* __restrict__ colors,
    const unsigned* __restrict__ counter, const uint4* __restrict__ mark, int live,
    const bdpt_dev_sphere* __restrict__ sph, int all_materials, float4* __restrict__ guide,
    float4* __restrict__ ping, int count) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    int g = id[i];
    if (g >= 0 && !all_materials && sph[g].refl != BDPT_DEV_DIFF) g = -1;
    const bdpt_dev_vec n = normal[i];
    guide[i] = make_float4(n.x, n.y, n.z, __int_as_float(g));
    const bdpt_dev_vec B = colors[i];
    float v0 = -1.0f;
    if (mark && live) {
        const uint4 rec = mark[i];
        const unsigned cnt = counter[i], mn = rec.w;
        // 2*(cnt - mn) >= mn without the overflow, as in bdpt_noise_kernel
        if (mn > 0u && cnt > mn && cnt - mn >= (mn >> 1) + (mn & 1u)) {
            const f3 d = sub(mk(B.x, B.y, B.z), mk(__uint_as_float(rec.x), __uint_as_float(rec.y), __uint_as_float(rec.z)));
            const float a = (float)mn, nf = (float)cnt;
            v0 = dot(d, d) * (a / (nf - a));
        }
    }
    ping[i] = make_float4(B.x, B.y, B.z, v0);
}

// The prefilter: one lane per pixel of a 32 x 8 tile; the tile's sphere ids and raw variances with
// a halo of 2 pixels are staged in LDS (8 B per position, loaded once per workgroup), the 25 taps
// are ds reads.  Positions outside the frame hold the id -2, which no eligible centre has.
extern "C" __global__ __launch_bounds__(256) void bdpt_dnoise_prefilter_kernel(const float4* __restrict__ guide,
                                                                                const float4* __restrict__ cur,
                                                                                float4* __restrict__ nxt, int W, int H) {
    __shared__ float2 sv0[BDPT_DNP_LDS_W * BDPT_DNP_LDS_H];   // {bits: id, v0}
    constexpr int rw = BDPT_DNP_LDS_W, rh = BDPT_DNP_LDS_H;
    const int bx0 = (int)blockIdx.x * BDPT_DN_BTW - 2, by0 = (int)blockIdx.y * BDPT_DN_BTH - 2;
    for (int k = threadIdx.x; k < rw * rh; k += 256) {
        const int ry = k / rw, rx = k - ry * rw;
        const int gx = bx0 + rx, gy = by0 + ry;
        float2 e = make_float2(__int_as_float(-2), -1.0f);
        if (gx >= 0 && gx < W && gy >= 0 && gy < H) e = make_float2(guide[gy * W + gx].w, cur[gy * W + gx].w);
        sv0[k] = e;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lx = wave * 8 + (lane & 7), ly = lane >> 3;
    const int x = (int)blockIdx.x * BDPT_DN_BTW + lx, y = (int)blockIdx.y * BDPT_DN_BTH + ly;
    if (x >= W || y >= H) return;
    const int i = y * W + x, li = (ly + 2) * rw + lx + 2;
    float4 rec = cur[i];
    const int gid = __float_as_int(sv0[li].x);
    if (gid >= 0) {
        constexpr float hk[5] = {1.f / 16.f, 1.f / 4.f, 3.f / 8.f, 1.f / 4.f, 1.f / 16.f};
        float sv = 0.f, sh = 0.f;
        bool used = false;
#pragma unroll
        for (int j = 0; j < 5; j++) {
#pragma unroll
            for (int t = 0; t < 5; t++) {
                const float2 e = sv0[li + (j - 2) * rw + (t - 2)];
                if (__float_as_int(e.x) != gid || e.y < 0.f) continue;
                sv = sv + (hk[j] * hk[t]) * e.y;
                sh = sh + hk[j] * hk[t];
                used = true;
            }
        }
        rec.w = used ? sv / sh : -1.0f;
    }
    nxt[i] = rec;
}

// ---------------------------------------------------------------------------------------------
// Temporal reprojection (include/bdpt.h bdpt_reproject; no reference counterpart).
// Host sequence on the context's stream: bdpt_aov_kernel (unjittered, whole frame, under the
// current camera), then bdpt_reproject_kernel; a capture also packs the planes into the next
// history's guide records.  Numerics as for the denoiser above: the definition operation for
// operation, fp32 without contraction, dot() as (x + y) + z, every reciprocal through rcp_rn
// (library division outside [2^-125, 2^125): cz = 0, a denormal sw), denormals kept.

// History records from planes: guide = {position, id} (either pair of pointers may be null).
extern "C" __global__ __launch_bounds__(256) void bdpt_history_pack_kernel(
    const int* __restrict__ id, const bdpt_dev_vec* __restrict__ position, const bdpt_dev_vec* __restrict__ colors,
    const float* __restrict__ weight, float4* __restrict__ guide, float4* __restrict__ col, int count) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    if (guide) {
        const bdpt_dev_vec p = position[i];
        guide[i] = make_float4(p.x, p.y, p.z, __int_as_float(id[i]));
    }
    if (col) {
        const bdpt_dev_vec c = colors[i];
        col[i] = make_float4(c.x, c.y, c.z, weight[i]);
    }
}

// One lane per pixel: the projection of the pixel's first-hit point into the history's camera,
// four validated taps of two 16-byte loads each (issued together; a tap outside the frame reads the
// lane's own record, always a valid address, and is not used), the blend, and the stores the call
// asked for.  Wave tiles 8 x 8 or 64 x 1 (v.rows), as in bdpt_aov_kernel.
extern "C" __global__ __launch_bounds__(256) void bdpt_reproject_kernel(bdpt_reproject_args v) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = v.rows ? (int)blockIdx.x * BDPT_RP_ROW_BTW + lane
                         : (int)blockIdx.x * BDPT_RP_BTW + wave * 8 + (lane & 7);
    const int y = v.rows ? (int)blockIdx.y * BDPT_RP_ROW_BTH + wave
                         : (int)blockIdx.y * BDPT_RP_BTH + (lane >> 3);
    if (x >= v.W || y >= v.H) return;                    // (no cross-lane operation below)
    const int i = y * v.W + x;
    const bdpt_dev_vec c3 = v.colors[i];
    const f3 c = mk(c3.x, c3.y, c3.z);
    const float n = (float)v.counter[i];
    const int id1 = v.id[i];
    bool eligible = v.hguide != nullptr && id1 >= 0;
    if (eligible && !v.all_materials) eligible = v.sph[id1].refl == BDPT_DEV_DIFF;
    float m = 0.f;
    f3 h = mk(0.f, 0.f, 0.f);
    if (eligible) {
        const bdpt_dev_vec p3 = v.position[i], n3 = v.normal[i];
        const f3 P = mk(p3.x, p3.y, p3.z), N = mk(n3.x, n3.y, n3.z);
        const f3 d = sub(P, mk(v.o[0], v.o[1], v.o[2]));
        const float a = dot(d, mk(v.ux[0], v.ux[1], v.ux[2]));
        const float b = dot(d, mk(v.uy[0], v.uy[1], v.uy[2]));
        const float cz = dot(d, mk(v.ud[0], v.ud[1], v.ud[2]));
        const float r = rcp_rn(cz);
        const float kx = (10.f * a) * r, ky = (10.f * b) * r;
        const float fx = (kx + v.hw) * v.sx, fy = (ky + v.hh) * v.sy;
        if (fx >= -1.f && fx < (float)v.W && fy >= -1.f && fy < (float)v.H) {   // a NaN fails
            const float xf = floorf(fx), yf = floorf(fy);
            const float wx = fx - xf, wy = fy - yf;
            const int qx0 = (int)xf, qy0 = (int)yf;       // -1 .. W-1, -1 .. H-1
            const float lim = v.plane_tol * v.t[i];
            float4 gq[4], cq[4];
            bool in[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int qx = qx0 + (k & 1), qy = qy0 + (k >> 1);
                in[k] = qx >= 0 && qx < v.W && qy >= 0 && qy < v.H;
                const int q = in[k] ? qy * v.W + qx : i;
                gq[k] = v.hguide[q];
                cq[k] = v.hcol[q];
            }
            float sw = 0.f, sm = 0.f;
            f3 sc = mk(0.f, 0.f, 0.f);
            bool used = false;
#pragma unroll
            for (int k = 0; k < 4; k++) {                 // dy outer, dx inner, as defined
                const float bx = (k & 1) ? wx : 1.f - wx, by = (k >> 1) ? wy : 1.f - wy;
                const float bw = bx * by;
                if (!in[k] || !(bw > 0.f) || __float_as_int(gq[k].w) != id1 || !(cq[k].w > 0.f)) continue;
                if (!(fabsf(dot(sub(mk(gq[k].x, gq[k].y, gq[k].z), P), N)) <= lim)) continue;
                sw = sw + bw;
                sm = sm + bw * fminf(cq[k].w, v.max_history);
                sc = add(sc, smul(bw, mk(cq[k].x, cq[k].y, cq[k].z)));
                used = true;
            }
            if (used) {
                h = smul(rcp_rn(sw), sc);
                m = sm;
            }
        }
    }
    const float tot = n + m;
    f3 o = c;
    if (m == 0.f) {
    } else if (n == 0.f) {
        o = h;
    } else {
        const float rt = rcp_rn(tot);
        o = mk((n * c.x + m * h.x) * rt, (n * c.y + m * h.y) * rt, (n * c.z + m * h.z) * rt);
    }
    if (v.next) v.next[i] = make_float4(o.x, o.y, o.z, v.clamp_next ? pv_clampc(tot) : tot);
    if (v.dn_guide) {                                    // the denoiser's guide record of the pixel
        int g = id1;
        if (g >= 0 && !v.all_materials && v.sph[g].refl != BDPT_DEV_DIFF) g = -1;
        const bdpt_dev_vec n3 = v.normal[i];
        v.dn_guide[i] = make_float4(n3.x, n3.y, n3.z, __int_as_float(g));
    }
    if (v.out3) {
        bdpt_dev_vec ov;
        ov.x = o.x; ov.y = o.y; ov.z = o.z;
        v.out3[i] = ov;
    }
    if (v.weight) v.weight[i] = tot;
    if (v.rgba) v.rgba[i] = bdpt_dev_to_rgba(o.x, o.y, o.z, v.gamma_thr);
}
// ---------------------------------------------------------------------------------------------
// Per-tile noise estimate from two frames (include/bdpt.h bdpt_noise_estimate; no
// reference counterpart).  One workgroup per 32 x 8 tile, thread index = slot, so a wave covers two
// frame rows of 32 pixels: its loads and stores are two contiguous runs each.  Memory bound: 12 + 4
// + 16 B read per pixel, 16 B written where a pixel takes the mark, 4 B with the per-pixel plane.
// The adjacent-pair tree of the definition runs as an xor butterfly in the wave's lanes (strides
// 1 .. 32: fp32 addition is commutative, so every lane, lane 0 among them, holds the value of the
// tree over the wave's 64 slots), the four wave partials meet in LDS as (p0 + p1) + (p2 + p3): the
// tree's last two rounds.  Counts are a ballot and a popcount per wave.  No atomics; the frame's
// summary is formed on the host from the tile arrays.  a / b is the compiler's correctly rounded
// division (denormals kept), the roots are bdpt_sqrt_rn.
extern "C" __global__ __launch_bounds__(256) void bdpt_noise_mark_kernel(const bdpt_dev_vec* __restrict__ colors,
                                                                         const unsigned* __restrict__ counter,
                                                                         uint4* __restrict__ mark, int np) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= np) return;
    const bdpt_dev_vec c = colors[i];
    mark[i] = make_uint4(__float_as_uint(c.x), __float_as_uint(c.y), __float_as_uint(c.z), counter[i]);
}

extern "C" __global__ __launch_bounds__(256) void bdpt_noise_kernel(bdpt_noise_args v) {
    __shared__ float part[4];
    __shared__ unsigned nvalid[4], npending[4];
    const int k = (int)threadIdx.x, lane = k & 63, wave = k >> 6;
    const int x = (int)blockIdx.x * BDPT_NOISE_BTW + (k & (BDPT_NOISE_BTW - 1));
    const int y = (int)blockIdx.y * BDPT_NOISE_BTH + k / BDPT_NOISE_BTW;
    float e = 0.f;                                       // an invalid slot adds +0
    bool ok = false, pending = false;
    if (x < v.W && y < v.H) {                            // (no return: the reduction below needs every lane)
        const int i = y * v.W + x;
        const bdpt_dev_vec B = v.colors[i];
        const unsigned cnt = v.counter[i];
        uint4 rec = make_uint4(0u, 0u, 0u, 0u);
        if (v.mark) rec = v.mark[i];
        const unsigned mn = v.live ? rec.w : 0u;
        // 2*(cnt - mn) >= mn without the overflow: cnt - mn >= ceil(mn / 2)
        ok = mn > 0u && cnt > mn && cnt - mn >= (mn >> 1) + (mn & 1u);
        const bool growing = cnt > 0u && cnt < BDPT_DEV_COUNTER_CAP;
        pending = growing && !ok;
        float pe = -1.0f;
        if (ok) {
            const float a = (float)mn, n = (float)cnt;
            const float dx = B.x - __uint_as_float(rec.x), dy = B.y - __uint_as_float(rec.y),
                        dz = B.z - __uint_as_float(rec.z);
            const float e1 = (fabsf(dx) + fabsf(dy)) + fabsf(dz);
            const float s = a / (n - a);
            const float f = bdpt_sqrt_rn(s);
            const float lum = (B.x + B.y) + B.z;
            const float den = bdpt_sqrt_rn(fmaxf(lum, v.dark));
            pe = (e1 * f) / den;
            e = pe;
        }
        if (v.error) v.error[i] = pe;
        if (v.remark) {                                  // cnt >= 2*mn as (cnt >> 1) >= mn
            const bool take = growing && (cnt >> 1) >= mn;
            // a cleared mark becomes live again with this call: a pixel that does not take it
            // keeps its colour and stores the count 0 it was read with
            if (take) v.mark[i] = make_uint4(__float_as_uint(B.x), __float_as_uint(B.y), __float_as_uint(B.z), cnt);
            else if (!v.live) v.mark[i] = make_uint4(rec.x, rec.y, rec.z, 0u);
        }
    }
    float s = e;
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) s = s + __shfl_xor(s, m, 64);
    const unsigned long long bv = __builtin_amdgcn_ballot_w64(ok), bp = __builtin_amdgcn_ballot_w64(pending);
    if (lane == 0) {
        part[wave] = s;
        nvalid[wave] = (unsigned)__popcll(bv);
        npending[wave] = (unsigned)__popcll(bp);
    }
    __syncthreads();
    if (k == 0) {
        const float S = (part[0] + part[1]) + (part[2] + part[3]);
        const unsigned c = (nvalid[0] + nvalid[1]) + (nvalid[2] + nvalid[3]);
        const int t = (int)blockIdx.y * v.tiles_x + (int)blockIdx.x;
        v.tile_sum[t] = S;
        v.tile_error[t] = c ? S / (float)c : 0.f;
        v.tile_valid[t] = c;
        v.tile_pending[t] = (npending[0] + npending[1]) + (npending[2] + npending[3]);
    }
}
