// bdpt_frame_kernels.h -- the kernels of the frame services (bdpt_frame.cpp): denoiser, temporal
// reprojection, denoised preview and noise estimate.  Part of bdpt_kernels.hip, which includes this
// file in its precompiled build only (never under BDPT_JIT), after the helpers used here: f3 and
// its operations, rcp_rn, bdpt_sqrt_rn, bdpt_dev_to_rgba, and bdpt_filter.h on the kernel side.
// bdpt_aov_kernel, whose planes these kernels read, stays there with the path kernel's traversal.
//
// What a pixel or a tap computes is stated once, in bdpt_filter.h, for these kernels and for the
// CPU backend (bdpt_cpu.cpp); this file is the device's driver of it: tiles, LDS staging, a row's
// loads batched before its taps, the wave reduction, and the launch tables.

// ---------------------------------------------------------------------------------------------
// Edge-avoiding wavelet denoiser (include/bdpt.h bdpt_denoise; no reference
// counterpart).  Host sequence on the context's stream: bdpt_aov_kernel (unjittered, whole frame),
// bdpt_denoise_pack_kernel, then one level kernel per level, ping-pong.
//
// Numerics: bdpt_filter.h with the device's reciprocals, both correctly rounded (rcp_rn:
// v_rcp_f32 + one Newton step inside [2^-125, 2^125), the library division outside, e.g. for
// 1 + e2 * isc = +inf).  Denormal intermediates are kept, not flushed: wn (a cosine squared up to
// six times) and w underflow gradually, and the build keeps fp32 denormals (hipcc's default for
// gfx9; the hipRTC flags of the specialised kernels say -fno-gpu-flush-denormals-to-zero
// explicitly).

// Guide records {normal, guide_id} and the first ping buffer.
extern "C" __global__ __launch_bounds__(256) void bdpt_denoise_pack_kernel(
    const int* __restrict__ id, const bdpt_dev_vec* __restrict__ normal, const bdpt_dev_vec* __restrict__ colors,
    const bdpt_dev_sphere* __restrict__ sph, int all_materials, float4* __restrict__ guide,
    float4* __restrict__ ping, int count) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const int g = guide_id(id[i], all_materials, sph);
    const bdpt_dev_vec n = normal[i];
    guide[i] = make_float4(n.x, n.y, n.z, __int_as_float(g));
    if (ping) {                                         // nullptr: the guide records alone
        const bdpt_dev_vec c = colors[i];
        ping[i] = make_float4(c.x, c.y, c.z, 0.f);
    }
}

// The level kernels of the three filters.  bdpt_preview_denoise (include/bdpt.h) runs
// bdpt_aov_kernel once, bdpt_reproject_kernel writing its {o, clampc(tot)} record into the ping
// buffer and the guide record next to it, then one level per level as the denoiser does: its level
// kernels are the denoiser's with the count in the colour record's .w (kLvCounts) -- the same
// 32-byte records, tiles and LDS staging.  bdpt_denoise_noise carries the variance
// there (kLvNoise).  The taps and finishes are bdpt_filter.h's (lv_tap, lv_finish).

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

// the mode's constant next to isc: c2 (counts) or s2 (noise)
template <int MODE, class Args>
__device__ __forceinline__ float level_k(const Args& v) {
    if constexpr (MODE == kLvCounts) return v.c2;
    else if constexpr (MODE == kLvNoise) return v.s2;
    else return 0.f;
}

// one tap that passed the id test, from its guide and colour records
template <int NP, int MODE, class Args>
__device__ __forceinline__ void level_tap(const Args& v, int j, int t, f3 n_p, f3 c_p, float a_p, float4 gq, float4 cq,
                                          float& su, float& sw, f3& sc, bool& used) {
    lv_tap<MODE>(b3_weight(j, t), NP, v.isc, level_k<MODE>(v), n_p, c_p, a_p, mk(gq.x, gq.y, gq.z),
                 mk(cq.x, cq.y, cq.z), cq.w, su, sw, sc, used);
}

template <int MODE, class Args>
__device__ __forceinline__ void level_finish(const Args& v, int i, bool used, f3 c_p, float a_p, float su, float sw,
                                             f3 sc) {
    float a;
    const f3 o = lv_finish<MODE>(used, c_p, a_p, su, sw, sc, a);
    level_store<MODE>(v, i, o, a);
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
                level_tap<NP, MODE>(v, j, t, n_p, c_p, a_p, gq[t], cq[t], su, sw, sc, used);
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
            level_tap<NP, MODE>(v, j, t, n_p, c_p, a_p, gq, scol[q], su, sw, sc, used);
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
// above, ping-pong from the prefilter's output.  Numerics as for the denoiser; bdpt_filter.h's
// a / (n - a) and sv / sh are the compiler's correctly rounded divisions (denormals kept).

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
    const int g = guide_id(id[i], all_materials, sph);
    const bdpt_dev_vec n = normal[i];
    guide[i] = make_float4(n.x, n.y, n.z, __int_as_float(g));
    const bdpt_dev_vec B = colors[i];
    float v0 = -1.0f;
    if (mark && live) {
        const uint4 rec = mark[i];
        const unsigned cnt = counter[i], mn = rec.w;
        const f3 A = mk(__uint_as_float(rec.x), __uint_as_float(rec.y), __uint_as_float(rec.z));
        // formed by every lane and kept where the mark is valid: the record stays one 16-byte load
        const float v = raw_variance(mk(B.x, B.y, B.z), A, cnt, mn);
        if (mark_valid(cnt, mn)) v0 = v;
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
        float sv = 0.f, sh = 0.f;
        bool used = false;
#pragma unroll
        for (int j = 0; j < 5; j++) {
#pragma unroll
            for (int t = 0; t < 5; t++) {
                const float2 e = sv0[li + (j - 2) * rw + (t - 2)];
                pf_tap(b3_weight(j, t), __float_as_int(e.x) == gid, e.y, sv, sh, used);
            }
        }
        rec.w = pf_finish(used, sv, sh);
    }
    nxt[i] = rec;
}

// ---------------------------------------------------------------------------------------------
// Temporal reprojection (include/bdpt.h bdpt_reproject; no reference counterpart).
// Host sequence on the context's stream: bdpt_aov_kernel (unjittered, whole frame, under the
// current camera), then bdpt_reproject_kernel; a capture also packs the planes into the next
// history's guide records.  Numerics as for the denoiser above: bdpt_filter.h's rp_project, rp_tap,
// rp_history and rp_blend with every reciprocal through rcp_rn (library division outside
// [2^-125, 2^125): cz = 0, a denormal sw), denormals kept.

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
// asked for.  Wave tiles 8 x 8 or 64 x 1 (v.rows), as in bdpt_aov_kernel.  With "follow"
// (v.hdelta: some sphere has moved since the history was taken) the lane first gathers its sphere's
// offset, one 16-byte load from a table the L1 holds, and projects and plane-tests
// the point shifted back by it (rp_follow).
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
    const int g1 = guide_id(id1, v.all_materials, v.sph);   // the pixel's sphere where it is eligible
    float m = 0.f;
    f3 h = mk(0.f, 0.f, 0.f);
    if (v.hguide != nullptr && g1 >= 0) {
        const bdpt_dev_vec p3 = v.position[i], n3 = v.normal[i];
        const f3 N = mk(n3.x, n3.y, n3.z);
        f3 P = mk(p3.x, p3.y, p3.z);
        if (v.hdelta != nullptr) {                        // "follow": where the pixel's sphere was (uniform branch)
            const float4 d = v.hdelta[id1];
            P = rp_follow(P, mk(d.x, d.y, d.z));
        }
        float fx, fy;
        if (rp_project(P, mk(v.o[0], v.o[1], v.o[2]), mk(v.ux[0], v.ux[1], v.ux[2]), mk(v.uy[0], v.uy[1], v.uy[2]),
                       mk(v.ud[0], v.ud[1], v.ud[2]), v.hw, v.hh, v.sx, v.sy, v.W, v.H, fx, fy)) {
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
            for (int k = 0; k < 4; k++)
                rp_tap(k, wx, wy, in[k], __float_as_int(gq[k].w), mk(gq[k].x, gq[k].y, gq[k].z),
                       mk(cq[k].x, cq[k].y, cq[k].z), cq[k].w, id1, P, N, lim, v.max_history, sw, sm, sc, used);
            rp_history(used, sw, sm, sc, h, m);
        }
    }
    float tot;
    const f3 o = rp_blend(c, n, h, m, tot);
    if (v.next) v.next[i] = make_float4(o.x, o.y, o.z, v.clamp_next ? clampc(tot) : tot);
    if (v.dn_guide) {                                    // the denoiser's guide record of the pixel
        const bdpt_dev_vec n3 = v.normal[i];
        v.dn_guide[i] = make_float4(n3.x, n3.y, n3.z, __int_as_float(g1));
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
// summary is formed on the host from the tile arrays.  The mark rules and the per-pixel error are
// bdpt_filter.h's: a / b is the compiler's correctly rounded division (denormals kept), the roots
// are bdpt_sqrt_rn.
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
        ok = mark_valid(cnt, mn);
        pending = mark_growing(cnt) && !ok;
        float pe = -1.0f;
        if (ok) {
            const f3 A = mk(__uint_as_float(rec.x), __uint_as_float(rec.y), __uint_as_float(rec.z));
            pe = pixel_error(mk(B.x, B.y, B.z), A, cnt, mn, v.dark);
            e = pe;
        }
        if (v.error) v.error[i] = pe;
        if (v.remark) {
            // a cleared mark becomes live again with this call: a pixel that does not take it
            // keeps its colour and stores the count 0 it was read with
            if (mark_take(cnt, mn))
                v.mark[i] = make_uint4(__float_as_uint(B.x), __float_as_uint(B.y), __float_as_uint(B.z), cnt);
            else if (!v.live)
                v.mark[i] = make_uint4(rec.x, rec.y, rec.z, 0u);
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
