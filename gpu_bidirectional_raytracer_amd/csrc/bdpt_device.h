// bdpt_device.h -- device-side data layout shared by the HIP kernels and the host launcher.
//
// HBM layout (one context = one GPU):
//   d_rand    float[7,684,096]      MT607 table, lane-major (tid + k*4096)      30.7 MB
//   d_rndp    float[29][307,364]    the same table in 29 planes (j mod 25)     35.6 MB
//   d_scp     float2[29][307,364]   {sinf, cosf}(2 pi u) of every d_rndp entry 71.3 MB
//             (filled before the first launch of a kernel that reads it: the pass-stream
//             kernels without sample records)
//   d_srec    float4[2][25][307,364] sample records (bdpt_sample_records_kernel): per table
//             position j, at [j mod 25][j / 25], half 0 = {A, B, C, u2}, half 1 = {X, Y, Z, u0}
//             (bdpt_math.h bdpt_sample_record); allocated and filled before the first launch
//             of a kernel that reads it (specialised pass-stream kernels, BDPT_SREC) 245.9 MB
//   d_lp      bdpt_dev_lightpath[4096]  VLPs {hp, rad, nl}, AoS 36 B            147 KB
//   d_sph     bdpt_dev_sphere[n]    48 B/sphere {p, rad^2, e, rad, c, refl}
//   d_colors  bdpt_dev_vec[W*H]     running-mean radiance, AoS 12 B (== dev_colors)
//   d_counter unsigned[W*H]         samples per pixel (== dev_counter)
//   d_pixels  uchar4[W*H]           gamma-2.2 8-bit RGBA (== pixels_buf)
//   d_aov     float[12][cap]        first-hit feature buffers (bdpt_aov_kernel): planes id, t, dp,
//             position, normal, dir of the largest window asked for; made on first use  48 B/pixel
//   d_chain   float[18][cap]        chain buffers (bdpt_chain_kernel): planes id, first_id, kind, bounces,
//             t, dp, position, normal, dir, throughput of the largest window asked for; made on
//             first use                                                              72 B/pixel
//   d_dn      float4[3][W*H]        denoiser (bdpt_denoise): guide records {normal, id or -1}, ping and
//             pong colours; made on the first call                                  48 B/pixel
//   d_hist    float4[4][W*H] + 20 B/pixel  reprojection (bdpt_reproject): two sets of history records
//             {gpos, gid}, {hc, hm} and the packed results; made on first use        84 B/pixel
//   d_hdelta  float4[n]             "follow" (bdpt_history_follow): the spheres' offsets from the
//             history's, written when a sphere has moved; made on first use          16 B/sphere
//   bdpt_preview_denoise works in d_dn (the count in the colour records' .w) and d_hist's results;
//   bdpt_denoise_noise works in d_dn (the variance in .w) and reads d_mark, the noise estimate's
//   uint4[W*H] records {mc, mn}; its packed results and variance plane go into d_aov
#ifndef BDPT_DEVICE_H
#define BDPT_DEVICE_H

#ifndef __HIPCC_RTC__                       // hipRTC provides the HIP runtime itself
#include <hip/hip_runtime.h>
#endif

#define BDPT_DEV_RAND_N (4096u * 1876u)
// d_Rand in 25 + 4 planes (bdpt_rand_planar_kernel): plane p < 25 holds d_Rand[25 q + p] at q,
// plane 25 + t holds d_Rand[25 (q + 1) + t]; PL = ceil(RAND_N / 25) entries per plane
#define BDPT_DEV_RANDP_PL 307364u
#define BDPT_DEV_RANDP_PLANES 29u
// sample records: 25 planes (the offsets +0..+4 are folded into the record: no wrap planes), two
// float4 halves BDPT_DEV_SREC_HALF entries apart; positions j >= RAND_N - 5 hold zeros
#define BDPT_DEV_SREC_HALF (25u * BDPT_DEV_RANDP_PL)
#define BDPT_DEV_N_PER_RNG 1876
#define BDPT_DEV_LIGHT_POINTS 4096
#define BDPT_DEV_COUNTER_CAP 30000u
#define BDPT_DEV_INLINE_PASSES 128      // launches of <= this many passes carry sid/vlp by value
#define BDPT_DEV_BVH_EMISSIVE (1 << 30)   // BVH sphere id flag (bdpt_bvh.h kBvhEmissive)
#define BDPT_DEV_DIFF 0
#define BDPT_DEV_SPEC 1
#define BDPT_DEV_REFR 2

// Path-kernel tiling: a wave covers BDPT_WTW x (64/BDPT_WTW) pixels, a 256-thread workgroup
// BDPT_BLOCK_WX x (4/BDPT_BLOCK_WX) waves (default 4x1: a 32x8 tile, so 8-row shard bands map to
// whole tile rows).  The host sizes the grid from the same macros.
#ifndef BDPT_WTW
#define BDPT_WTW 8
#endif
#ifndef BDPT_BLOCK_WX
#define BDPT_BLOCK_WX 4
#endif
#define BDPT_WTH (64 / BDPT_WTW)
#define BDPT_BLOCK_WY (4 / BDPT_BLOCK_WX)
#define BDPT_BTW (BDPT_BLOCK_WX * BDPT_WTW)
#define BDPT_BTH (BDPT_BLOCK_WY * BDPT_WTH)

struct bdpt_dev_vec { float x, y, z; };
struct bdpt_dev_lightpath { float hx, hy, hz, rx, ry, rz, nx, ny, nz; };
struct bdpt_dev_sphere {
    float px, py, pz, rr;     // rr = rad*rad (the float product SphereIntersectDevice forms)
    float ex, ey, ez, rad;
    float cx, cy, cz;
    int refl;
};

struct bdpt_path_args {
    const bdpt_dev_sphere* sph;
    unsigned n;
    unsigned n_lights;
    const int* lights;              // indices of emitters (e != 0), ascending
    const float4* lightrec;         // per emitter: {p, rad}, {e, (4*pi*rad)*rad}
    const float4* geom;             // per sphere {p, rad*rad} (SGPR-resident traversal)
    const float4* vgeom;            // the non-emitters' {p, rad*rad}, ascending index (n_vac of them):
    int n_vac;                      // the sphere list of a VLP-only shadow round
    unsigned emis_mask;             // bit s = sphere s is emissive (sphere counts <= 32)
    const float* rnd;
    const float* rndp;              // the planar copy (BDPT_DEV_RANDP_*), pass-stream kernels
    const float2* scp;              // per planar entry u: {sinf, cosf}(2 pi u) (bdpt_sincos_planar_kernel);
                                    // for a BDPT_SREC kernel the sample records instead (d_srec, float4)
    const bdpt_dev_lightpath* lp;
    const unsigned* sid;            // per pass (nullptr: the pass table is sid_inl / vlp_inl)
    const int* vlp;                 // per pass
    int npass;
    // a launch of <= BDPT_DEV_INLINE_PASSES passes (every launch of bdpt_path_passes) carries its
    // pass table in the arguments: no upload, no copy kernel before the path kernel
    unsigned sid_inl[BDPT_DEV_INLINE_PASSES];
    int vlp_inl[BDPT_DEV_INLINE_PASSES];
    bdpt_dev_vec* colors;
    unsigned* counter;
    uchar4* pixels;
    const float* gamma_thr;         // 256 thresholds of toInt (vec.h:34)
    int W, H;
    float inv_w, inv_h;             // (float)(14./W), (float)(10.5/H)
    double half_w, half_h;          // (double)(inv_w*W)/2., (double)(inv_h*H)/2.
    float ux[3], uy[3], ud[3], orig[3];
    float tx, ty, tz;
    int shard, nshards, band_rows;
    int tiles_per_band;             // > 0: grid rows enumerate only this shard's bands
    int streams;                    // pass streams S: lane (pixel, s) renders passes s, s+S, ...
    bdpt_dev_vec* rbuf;             // S > 1: per (pass, launched pixel) radiance, [npass][nloc]
    unsigned* rmask;                // pixel pools: per launched pixel 4 words, bit p set = rbuf holds
                                    // pass p's sample (clear: its radiance is +0, not stored)
    int nloc;                       // launched pixels per pass = tile-grid rows * BDPT_BTH * W
    int pool;                       // > 0 (BDPT_POOL builds): a wave renders one pass, restarting lanes
                                    // on new pixels, claimed in chunks of pool x 64 launched pixels
    unsigned* pool_ctr;             // per pass of the launch and eighth of its pixels: pixels claimed,
                                    // one 128-B line each (zero at the launch's start)
    unsigned* pool_ctr_next;        // the next pooled launch's counters: this launch zeroes them
    // BVH traversal (large scenes, kernel table index 17; see bdpt_bvh.cpp)
    const float4* bvh_nodes;        // 2 per node: {lo, skip}, {hi, leaf first|count<<24 or -1}
    const float4* bvh_geom;         // BVH spheres in leaf order {p, rad^2}
    const int* bvh_ids;             // sphere index | 1<<30 if emissive
    const float4* big_geom;         // brute-force spheres (walls) {p, rad^2}
    const int* big_ids;
    const float4* mat;              // per sphere: {c, refl | emissive<<8}, {e, rad}, {p, 0}
    int bvh_nn, bvh_ns, big_n;
    float bvh_c[3], bvh_r;          // ball around every BVH sphere (per-ray margin)
    float bvh_q;                    // 64u / smallest BVH radius (per-ray margin)
    unsigned long long* prof;       // BDPT_PROF builds: per-section shader cycles (8 counters)
    // Ordered in-kernel fold (BDPT_UNITS builds of the pass-stream kernel): a workgroup claims a
    // unit (tile, range) = passes [range * unit_passes, ...) of a 32x8 tile, one lane per pixel,
    // with the running mean in registers; the units of a tile run in range order (a wave waits for
    // its 8x8 tile's flag to reach epoch << 8 | range).
    int unit_passes;                // passes per range
    int unit_wgs;                   // tile workgroups of the launch (gx * gy)
    int gx, gy;                     // the tile grid the 1-D unit grid enumerates
    unsigned unit_tag;              // this launch's epoch << 8
    unsigned* unit_flags;           // per 8x8 wave tile: epoch << 8 | ranges folded
    unsigned* unit_err;             // non-zero: a handover wait timed out (ordering violated)
    unsigned* unit_ctr;             // per XCD queue: units claimed (8 counters, 128 B apart, zeroed per launch)
    int unit_taper;                 // 1: the launch's last unit_passes passes in halving ranges
    // Tile list (bdpt_path_passes_tiles; not pools, not units): workgroup b of the launch's x
    // dimension renders tile tile_list[b] of the gx x gy tile grid (row-major), and the launch's
    // pixel b * 256 + slot is that tile's slot (bdpt_dev_list_* below), inside the frame or
    // not: nloc = 256 * ntiles.  nullptr: the grid enumerates every tile itself.
    const unsigned* tile_list;
    int ntiles;
};

// First-hit feature buffers (bdpt_aov_kernel; include/bdpt.h bdpt_render_aov): the window, the
// jitter and the output planes, packed [h][w].  The scene, the camera constants, the random table
// and the BVH come from the bdpt_path_args the kernel also receives.
struct bdpt_aov_args {
    int x0, y0, w, h;               // the window inside the W x H frame (checked by the host)
    int jitter;                     // 0: both camera randoms are +0.0f (a.rnd is not read)
    unsigned sid;                   // kk = (26 + 25 i + sid) mod (RAND_N - 5), device.cu:562
    int bvh;                        // 1: walls brute force + BVH (a.bvh_*), 0: the n-sphere scan
    int rows;                       // 1: a wave covers 64 x 1 pixels, 0: 8 x 8 (below)
    int* id;                       // sphere index, -1 = miss
    float* t;
    float* dp;
    bdpt_dev_vec* position;
    bdpt_dev_vec* normal;
    bdpt_dev_vec* dir;
};
// Wave tiles of the feature-buffer kernel: 8 x 8 pixels when the BVH is traversed (coherent rays,
// as in the path kernel), 64 x 1 for the brute scan (no divergence to contain; row-contiguous
// stores).  A 256-thread workgroup covers 32 x 8 or 64 x 4 pixels.
#define BDPT_AOV_BVH_BTW 32
#define BDPT_AOV_BVH_BTH 8
#define BDPT_AOV_ROW_BTW 64
#define BDPT_AOV_ROW_BTH 4

// The eye path up to its first non-specular vertex (bdpt_chain_kernel; include/bdpt.h
// bdpt_render_chain): bdpt_aov_kernel's window, jitter and traversal, the glass rule, and the ten
// output planes, packed [h][w].  key_n > 0 (the denoisers' "through" guides): the id plane holds the
// guide key of include/bdpt.h BDPT_DENOISE_THROUGH instead -- -1 unless the chain ends DIFFUSE.
#define BDPT_DEV_CHAIN_DIFFUSE 0
#define BDPT_DEV_CHAIN_EMITTER 1
#define BDPT_DEV_CHAIN_MISS 2
#define BDPT_DEV_CHAIN_EXHAUSTED 3
struct bdpt_chain_args {
    int x0, y0, w, h;               // the window inside the W x H frame (checked by the host)
    int jitter;                     // 0: both camera randoms are +0.0f
    unsigned sid;
    int bvh;                        // 1: walls brute force + BVH (a.bvh_*), 0: the n-sphere scan
    int rows;                       // 1: a wave covers 64 x 1 pixels, 0: 8 x 8
    int pass;                       // 0: glass transmits whenever it can; 1: rnd[j + 2] < P reflects
    int key_n;                      // 0: id is the end sphere; n: id is the guide key
    const bdpt_dev_sphere* sph;     // materials (a per-lane load at the hit sphere's index)
    int* id;
    int* first_id;
    int* kind;
    int* bounces;
    float* t;
    float* dp;
    bdpt_dev_vec* position;
    bdpt_dev_vec* normal;
    bdpt_dev_vec* dir;
    bdpt_dev_vec* throughput;
};
#define BDPT_CHAIN_WORDS 18         // words per pixel of the ten planes

// Edge-avoiding wavelet denoiser (bdpt_denoise_pack_kernel / bdpt_denoise_level_kernel;
// include/bdpt.h bdpt_denoise).  Context-owned, 48 B per pixel, made on the first call:
//   guide  float4[W*H]  {normal, bits: the first hit's sphere id, or -1 for an ineligible pixel}
//   ping / pong  float4[W*H]  the level's input / output colour in xyz (w unused)
// One level launch reads `cur` and `guide` and writes `nxt`; the last one may write the packed
// results instead (out3: bdpt_dev_vec[W*H], rgba: uchar4[W*H]; either may be nullptr).
struct bdpt_denoise_args {
    int W, H;
    int step;                       // 2^k
    float isc;                      // isc_0 * 4^k
    int normal_power;               // squarings of the normal weight, 0..6
    int rows;                       // 1: a wave covers 64 x 1 pixels, 0: 8 x 8
    const float4* guide;
    const float4* cur;
    float4* nxt;                    // nullptr on a last level that only writes out3 / rgba
    bdpt_dev_vec* out3;
    uchar4* rgba;
    const float* gamma_thr;
};
// Workgroup tiles of the level kernel, as for the feature buffers: 32 x 8 (four 8 x 8 waves) or
// 64 x 4 (four rows).  The LDS variant stages a 32 x 8 tile plus a halo of 2 * step <= 4 pixels.
#define BDPT_DN_BTW 32
#define BDPT_DN_BTH 8
#define BDPT_DN_ROW_BTW 64
#define BDPT_DN_ROW_BTH 4
#define BDPT_DN_LDS_MAX_STEP 2
#define BDPT_DN_LDS_W (BDPT_DN_BTW + 4 * BDPT_DN_LDS_MAX_STEP)
#define BDPT_DN_LDS_H (BDPT_DN_BTH + 4 * BDPT_DN_LDS_MAX_STEP)

// The reprojected preview, denoised with per-pixel counts (bdpt_preview_level_t; include/bdpt.h
// bdpt_preview_denoise).  The denoiser's records and tiles: `cur` / `nxt` are {colour, count a};
// the last level may write the packed results (out3, weight, rgba; any may be nullptr).
struct bdpt_preview_args {
    int W, H;
    int step;                       // 2^k
    float isc;                      // isc_0 * 4^k
    float c2;                       // 2.f / count_ref
    int rows;                       // 1: a wave covers 64 x 1 pixels, 0: 8 x 8
    const float4* guide;
    const float4* cur;
    float4* nxt;                    // nullptr on a last level
    bdpt_dev_vec* out3;
    float* weight;
    uchar4* rgba;
    const float* gamma_thr;
};

// The noise-guided denoiser (bdpt_dnoise_pack_kernel, bdpt_dnoise_prefilter_kernel, bdpt_dnoise_level_t;
// include/bdpt.h bdpt_denoise_noise).  The denoiser's records and tiles: `cur` / `nxt` are {colour,
// variance v, -1: none}; the pack kernel writes {B, raw v0} into ping, the prefilter reads it and
// writes {B, v} into pong, where the levels start.  The last level may write the packed results
// (out3, variance: float[W*H], rgba; any may be nullptr).
struct bdpt_dnoise_args {
    int W, H;
    int step;                       // 2^k
    float isc;                      // isc_0 * 4^k
    float s2;                       // noise_sigma^2
    int rows;                       // 1: a wave covers 64 x 1 pixels, 0: 8 x 8
    const float4* guide;
    const float4* cur;
    float4* nxt;                    // nullptr on a last level
    bdpt_dev_vec* out3;
    float* variance;
    uchar4* rgba;
    const float* gamma_thr;
};
#define BDPT_DEV_DNOISE_EPS 1e-12f      // BDPT_DENOISE_NOISE_EPS (include/bdpt.h)
// the prefilter stages a 32 x 8 tile and its halo of 2 pixels: sphere id and raw variance
#define BDPT_DNP_LDS_W (BDPT_DN_BTW + 4)
#define BDPT_DNP_LDS_H (BDPT_DN_BTH + 4)

// Temporal reprojection (bdpt_history_pack_kernel / bdpt_reproject_kernel; include/bdpt.h
// bdpt_reproject).  Context-owned history, made on first use: two sets (ping-pong: a capture reads
// one and writes the other) of
//   guide  float4[W*H]  {gpos, bits: gid}   position and sphere id of C0's unjittered first hit
//   col    float4[W*H]  {hc, hm}            colour and weight
// = 2 x 32 B per pixel, plus the packed results of a call (out3 12 B, weight 4 B, rgba 4 B).
// The current view's first hit comes from the planes bdpt_aov_kernel has just written.
struct bdpt_reproject_args {
    int W, H;
    int rows;                       // 1: a wave covers 64 x 1 pixels, 0: 8 x 8
    int all_materials;              // 0: only pixels showing a DIFF sphere take history
    float max_history, plane_tol;
    float ux[3], uy[3], ud[3], o[3];   // C0 (camera_args of the history's camera)
    float hw, hh, sx, sy;
    const int* id;                  // the current camera's first hit (d_aov planes)
    const float* t;
    const bdpt_dev_vec* position;
    const bdpt_dev_vec* normal;
    const bdpt_dev_sphere* sph;
    const bdpt_dev_vec* colors;
    const unsigned* counter;
    const float4* hguide;           // nullptr: no history present (out = colors, weight = counter)
    const float4* hcol;
    // "follow" (bdpt_history_follow): {delta[k], 0} per sphere, the offsets of the context's spheres
    // from the history's; nullptr unless follow is on and some sphere has moved (BDPT_HISTORY_MOVED)
    const float4* hdelta;
    float4* next;                  // capture: the next history's {colour, weight} records
    bdpt_dev_vec* out3;             // any of these may be nullptr
    float* weight;
    uchar4* rgba;
    const float* gamma_thr;
    // bdpt_preview_denoise only (nullptr / 0 otherwise): the denoiser's guide record {normal, bits:
    // id1 or -1 for an ineligible pixel} of the pixel, and `next`'s count through clampc
    float4* dn_guide;
    int clamp_next;
};
#define BDPT_RP_BTW 32
#define BDPT_RP_BTH 8
#define BDPT_RP_ROW_BTW 64
#define BDPT_RP_ROW_BTH 4

// bdpt_noise_kernel (include/bdpt.h bdpt_noise_estimate): one 256-thread workgroup per
// BDPT_NOISE_BTW x BDPT_NOISE_BTH tile (the path kernel's workgroup tile), thread index = slot.
struct bdpt_noise_args {
    int W, H, tiles_x;
    int live;                       // 0: the mark is cleared (every mn reads 0, whatever is stored)
    int remark;
    float dark;
    const bdpt_dev_vec* colors;
    const unsigned* counter;
    uint4* mark;                    // {mc.x, mc.y, mc.z, mn} per pixel; nullptr: none allocated
    float* error;                   // W*H plane, or nullptr
    float* tile_sum;                // S_t, E_t, c_t and the pending count per tile
    float* tile_error;
    unsigned* tile_valid;
    unsigned* tile_pending;
};
#define BDPT_NOISE_BTW 32
#define BDPT_NOISE_BTH 8

// Units' pass ranges: unit_passes (P) passes each, except (taper) the launch's last <= P passes,
// which are split in halves -- P = 8: ..., 8, 4, 2, 1, 1 -- so that the launch drains over short
// units (the tiles' last ranges are what runs while the chip empties).  Range r starts at the
// returned pass and holds *len passes; bdpt_unit_ranges counts them.
__host__ __device__ inline int bdpt_unit_range(int npass, int P, int taper, int r, int* len) {
    if (!taper) {
        const int s = r * P;
        *len = npass - s < P ? npass - s : P;
        return s;
    }
    const int nbig = (npass - 1) / P;
    if (r < nbig) {
        *len = P;
        return r * P;
    }
    int s = nbig * P, T = npass - s;
    for (int t = r - nbig; t > 0; t--) {
        const int h = (T + 1) / 2;
        s += h;
        T -= h;
    }
    *len = T > 1 ? (T + 1) / 2 : T;
    return s;
}
__host__ __device__ inline int bdpt_unit_ranges(int npass, int P, int taper) {
    if (!taper) return (npass + P - 1) / P;
    const int nbig = (npass - 1) / P;
    int T = npass - nbig * P, n = nbig;
    while (T > 0) {
        T -= T > 1 ? (T + 1) / 2 : 1;
        n++;
    }
    return n;
}

// Tile row of a workgroup row: identity, or the sub-th tile row of this shard's k-th band.
__device__ __forceinline__ int bdpt_dev_tile_row(const bdpt_path_args& a, int by) {
    if (a.tiles_per_band <= 0) return by;
    if (a.tiles_per_band == 1) return a.shard + by * a.nshards;   // 8-row bands (the default)
    const int k = by / a.tiles_per_band, sub = by - k * a.tiles_per_band;
    return (a.shard + k * a.nshards) * a.tiles_per_band + sub;
}

// Launch-local pixel index under a tile list (bdpt_path_args::tile_list), the one statement of it:
// list entry b is tile (bx, by), and its pixel (x, y) is the launch's pixel
//   b * 256 + (y - by * BDPT_BTH) * BDPT_BTW + (x - bx * BDPT_BTW)
// -- the tile's 256 slots row-major, whether inside the frame or not.  The path kernel forms it as
// (y - row0) * BDPT_BTW + x with the wave-uniform row0 = bdpt_dev_list_row0(b, bx, by), the shape
// of its index without a list, (y - yoff) * W + x; the fold inverts it with bdpt_dev_list_pixel.
static_assert(BDPT_BTW * BDPT_BTH == 256, "a workgroup tile is 256 pixels");
__host__ __device__ __forceinline__ int bdpt_dev_list_row0(int b, int bx, int by) {
    return (by - b) * BDPT_BTH + bx;          // BTW * ((b - by) * BTH - bx) = b * 256 - by * BTH * BTW - bx * BTW
}
__host__ __device__ __forceinline__ void bdpt_dev_list_pixel(int bx, int by, int slot, int* x, int* y) {
    *x = bx * BDPT_BTW + slot % BDPT_BTW;
    *y = by * BDPT_BTH + slot / BDPT_BTW;
}

// toInt (vec.h:34) by threshold search: thr[k] is the smallest float whose toInt is >= k,
// computed on the host with the same pow as the reference semantics; 8 compares per channel.
__device__ __forceinline__ int bdpt_dev_gamma8(float v, const float* __restrict__ thr) {
    int k = 0;
#pragma unroll
    for (int step = 128; step > 0; step >>= 1)
        if (v >= thr[k + step]) k += step;
    return k;
}

__device__ __forceinline__ uchar4 bdpt_dev_to_rgba(float r, float g, float b,
                                                   const float* __restrict__ thr) {
    uchar4 o;
    o.x = (unsigned char)bdpt_dev_gamma8(r, thr);
    o.y = (unsigned char)bdpt_dev_gamma8(g, thr);
    o.z = (unsigned char)bdpt_dev_gamma8(b, thr);
    o.w = 0;
    return o;
}

#endif
