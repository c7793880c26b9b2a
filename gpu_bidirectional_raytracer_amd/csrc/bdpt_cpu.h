// bdpt_cpu.h -- the host (CPU) backend behind the C-ABI (bdpt_create with BDPT_DEVICE_CPU).
// Internal interface between bdpt_host.cpp and bdpt_cpu.cpp; no HIP in either signature.
#ifndef BDPT_CPU_H
#define BDPT_CPU_H

#include <stddef.h>
#include <stdint.h>

#include "../../include/bdpt.h"

struct bdpt_cpu_ctx;

bdpt_cpu_ctx* bdpt_cpu_create(const bdpt_sphere* spheres, unsigned n, int W, int H, const uint32_t* mt_params);
void bdpt_cpu_destroy(bdpt_cpu_ctx* c);
void bdpt_cpu_set_scene(bdpt_cpu_ctx* c, const bdpt_sphere* spheres, unsigned n);
void bdpt_cpu_set_camera(bdpt_cpu_ctx* c, const bdpt_camera* cam);
void bdpt_cpu_reset_accum(bdpt_cpu_ctx* c);
void bdpt_cpu_set_shard(bdpt_cpu_ctx* c, int shard, int nshards, int band_rows);
int bdpt_cpu_threads(const bdpt_cpu_ctx* c);
void bdpt_cpu_generate_rand(bdpt_cpu_ctx* c, unsigned seed);
void bdpt_cpu_light_pass(bdpt_cpu_ctx* c, int current_sample);
// tile_mask (include/bdpt.h bdpt_path_passes_tiles): one byte per BDPT_NOISE_TW x BDPT_NOISE_TH tile,
// row-major; only pixels of tiles with a non-zero byte are rendered.  nullptr: every pixel.
void bdpt_cpu_path_passes(bdpt_cpu_ctx* c, const unsigned* sid, const int* vlp, int npass,
                          const unsigned char* tile_mask = nullptr);
void bdpt_cpu_render_aov(const bdpt_cpu_ctx* c, int x0, int y0, int w, int h, int jitter, unsigned sid,
                         const bdpt_aov_buffers* out);
// the eye path up to its first non-specular vertex (include/bdpt.h bdpt_render_chain); the caller has
// checked the window, the branch, the camera and (jitter) the table
void bdpt_cpu_render_chain(const bdpt_cpu_ctx* c, int x0, int y0, int w, int h, int jitter, unsigned sid, int branch,
                           const bdpt_chain_buffers* out);
// materials = BDPT_DENOISE_THROUGH: the largest guide key, 6 n^2 + n - 1, must fit an int
// (include/bdpt.h: a scene with 6 n^2 + n > 2^31 - 1 is refused)
inline bool bdpt_chain_keys_fit(unsigned n) {
    return 6ull * n * n + n <= 0x7fffffffull;
}
void bdpt_cpu_denoise(const bdpt_cpu_ctx* c, const bdpt_denoise_params* p, bdpt_vec* colors_out,
                      unsigned char* rgba_out);
// temporal reprojection (include/bdpt.h bdpt_reproject); the caller has checked parameters and camera
bool bdpt_cpu_history_present(const bdpt_cpu_ctx* c);                       // stored and usable (state 1, or 2 with follow on)
// "follow" (include/bdpt.h bdpt_history_follow / bdpt_history_motion): the switch, and the state
// BDPT_HISTORY_* with the offsets (delta: one per sphere of the context, or nullptr)
void bdpt_cpu_history_follow(bdpt_cpu_ctx* c, int on);
int bdpt_cpu_history_motion(const bdpt_cpu_ctx* c, bdpt_vec* delta);
// the state of a history (`stored`) taken under s0[n0] against the spheres s[n], and the offsets in
// the states SAME and MOVED: host code shared by both backends
int bdpt_history_state(bool stored, const bdpt_sphere* s0, size_t n0, const bdpt_sphere* s, size_t n, bdpt_vec* delta);
bool bdpt_cpu_history_stored(const bdpt_cpu_ctx* c, bdpt_camera* cam);     // stored at all; *cam = C0 then
void bdpt_cpu_history_clear(bdpt_cpu_ctx* c);
void bdpt_cpu_history_read(const bdpt_cpu_ctx* c, bdpt_vec* colors, float* weight);
void bdpt_cpu_history_write(bdpt_cpu_ctx* c, const bdpt_camera* cam, const bdpt_vec* colors, const float* weight);
void bdpt_cpu_history_capture(bdpt_cpu_ctx* c, const bdpt_reproject_params* p);
void bdpt_cpu_reproject(const bdpt_cpu_ctx* c, const bdpt_reproject_params* p, bdpt_vec* colors_out,
                        float* weight_out, unsigned char* rgba_out);
// count-weighted denoising of the reprojected preview (include/bdpt.h bdpt_preview_denoise)
void bdpt_cpu_preview_denoise(const bdpt_cpu_ctx* c, const bdpt_preview_params* p, bdpt_vec* colors_out,
                              float* weight_out, unsigned char* rgba_out);
// per-tile noise estimate (include/bdpt.h bdpt_noise_estimate); the caller has checked the parameters.
// tile_sum / tile_error / tile_valid / tile_pending: S_t, E_t, c_t and the pending count per tile,
// tiles_x * tiles_y each; any output may be NULL
bool bdpt_cpu_noise_stored(const bdpt_cpu_ctx* c);                          // a mark was ever stored
void bdpt_cpu_noise_mark(bdpt_cpu_ctx* c);
void bdpt_cpu_noise_clear(bdpt_cpu_ctx* c);
void bdpt_cpu_noise_read_mark(const bdpt_cpu_ctx* c, bdpt_vec* colors, unsigned* counter);
void bdpt_cpu_noise_write_mark(bdpt_cpu_ctx* c, const bdpt_vec* colors, const unsigned* counter);
void bdpt_cpu_noise_estimate(bdpt_cpu_ctx* c, const bdpt_noise_params* p, float* error_out, float* tile_sum,
                             float* tile_error, unsigned* tile_valid, unsigned* tile_pending);
// noise-guided denoiser (include/bdpt.h bdpt_denoise_noise); the caller has checked parameters and camera
void bdpt_cpu_denoise_noise(const bdpt_cpu_ctx* c, const bdpt_denoise_noise_params* p, bdpt_vec* colors_out,
                            unsigned char* rgba_out, float* variance_out);
// the last estimate's pending count per tile (bdpt_noise_tile_pending); false before the first estimate
bool bdpt_cpu_noise_tile_pending(const bdpt_cpu_ctx* c, unsigned* tile_pending);
// the frame's summary from the tile arrays: host code shared by both backends
void bdpt_noise_summarize(const float* tile_sum, const float* tile_error, const unsigned* tile_valid,
                          const unsigned* tile_pending, int tiles_x, int tiles_y, float threshold,
                          bdpt_noise_summary* out);
bool bdpt_cpu_rand_ready(const bdpt_cpu_ctx* c);
bool bdpt_cpu_camera_set(const bdpt_cpu_ctx* c);
void bdpt_cpu_read_radiance(const bdpt_cpu_ctx* c, bdpt_vec* colors, unsigned* counter);
void bdpt_cpu_read_pixels(const bdpt_cpu_ctx* c, unsigned char* rgba);
void bdpt_cpu_read_rand(const bdpt_cpu_ctx* c, float* t);
void bdpt_cpu_write_rand(bdpt_cpu_ctx* c, const float* t);
void bdpt_cpu_read_lightpaths(const bdpt_cpu_ctx* c, bdpt_lightpath* lp);
void bdpt_cpu_write_lightpaths(bdpt_cpu_ctx* c, const bdpt_lightpath* lp);
void bdpt_cpu_update_pixels(bdpt_cpu_ctx* c);
void bdpt_cpu_write_radiance(bdpt_cpu_ctx* c, const bdpt_vec* colors, const unsigned* counter);

#endif
