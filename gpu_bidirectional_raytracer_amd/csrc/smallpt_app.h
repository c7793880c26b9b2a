/*
 * smallpt_app.h -- the host state and the reference's host-side operations shared by the headless
 * host (smallpt.c) and the optional display (smallpt_gl.c): UpdateRendering / UpdateRendering2
 * (smallpt_cpu.c:265-362), ReInit / ReInitScene (:365-387), SavePPM (:238-262) and the
 * KeyFunc / SpecialFunc dispatch (display_func.c:278-437) over the C-ABI of include/bdpt.h.
 */
#ifndef SMALLPT_APP_H
#define SMALLPT_APP_H

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/time.h>

#include "../../include/bdpt.h"

static double wall_clock(void)                            /* WallClockTime display_func.c:61 */
{
    struct timeval t;
    gettimeofday(&t, NULL);
    return t.tv_sec + t.tv_usec / 1000000.0;
}

typedef struct {
    bdpt_ctx *ctx;
    bdpt_camera camera;
    bdpt_sphere *spheres;
    unsigned n;
    int width, height;
    int current_sample, reinit_counter, current_sphere;
    float total_time;
    bdpt_pass_state ps;
    int reuse_history;                 /* --reproject: camera keys capture the frame before ReInit */
    int follow_spheres;                /* --reproject-follow: sphere and selection keys capture it too */
    bdpt_reproject_params rp;
} host;

static void report(host *h, int rc, const char *what)
{
    if (rc != BDPT_OK) fprintf(stderr, "%s failed: %s\n", what, bdpt_last_error(h->ctx));
}

/* UpdateRendering2 smallpt_cpu.c:300-362 */
static void update_rendering2(host *h)
{
    printf("UpdateRendering2\n");
    report(h, bdpt_light_pass(h->ctx, h->current_sample), "Kernel Light Tracing");
    bdpt_pass_state_light(&h->ps);
}

/* npass x UpdateRendering smallpt_cpu.c:265-297, fused into one launch; with a tile mask
 * (bdpt_path_passes_tiles, no reference counterpart) only the `pixels` pixels of the masked-in
 * tiles are rendered and counted, while the pass schedule and current_sample advance all the same */
static void update_rendering_tiles(host *h, int npass, const unsigned char *tile_mask, long long pixels)
{
    unsigned *sid = malloc(sizeof(unsigned) * npass);
    int *vlp = malloc(sizeof(int) * npass);
    bdpt_pass_schedule(&h->ps, npass, sid, vlp);
    double start = wall_clock();
    int rc = bdpt_path_passes_tiles(h->ctx, sid, vlp, npass, tile_mask);
    if (rc == BDPT_OK) rc = bdpt_synchronize(h->ctx);
    report(h, rc, "Kernel RadiancePathTracing");
    h->current_sample += npass;
    const float elapsed = (float)(wall_clock() - start);
    h->total_time += elapsed;
    const float sample_sec = (tile_mask ? (float)pixels : (float)h->height * h->width) * npass / elapsed;
    printf("Rendering time %.3f sec (pass %d) Total:%.2f  Sample/sec  %.1fK\n", elapsed,
           h->current_sample, h->total_time, sample_sec / 1000.f);
    free(sid);
    free(vlp);
}

static void update_rendering(host *h, int npass)
{
    update_rendering_tiles(h, npass, NULL, 0);
}

/* ReInit smallpt_cpu.c:373-387 (buffers persist; only the accumulation restarts) */
static void reinit(host *h)
{
    report(h, bdpt_reset_accum(h->ctx), "ReInit");
    h->reinit_counter++;
    bdpt_update_camera(&h->camera, h->width, h->height);
    report(h, bdpt_set_camera(h->ctx, &h->camera), "ReInit camera");
    h->current_sample = 0;
    if (h->reinit_counter % 2 == 0) update_rendering2(h);
    update_rendering(h, 1);
}

/* ReInitScene smallpt_cpu.c:365-371 */
static void reinit_scene(host *h)
{
    /* the context still holds the old spheres: with --reproject-follow the frame becomes the history,
     * which then follows the moved sphere (bdpt_history_follow) */
    if (h->follow_spheres) report(h, bdpt_history_capture(h->ctx, &h->rp), "ReInitScene history capture");
    else if (h->reuse_history) report(h, bdpt_history_clear(h->ctx), "ReInitScene history");
    h->current_sample = 0;
    report(h, bdpt_reset_accum(h->ctx), "ReInitScene");
    report(h, bdpt_set_scene(h->ctx, h->spheres, h->n), "ReInitScene upload");
    update_rendering2(h);
}

/* SavePPM smallpt_cpu.c:238-262 ('p' in KeyFunc): reference file name, ASCII P3 */
static int save_ppm(host *h, const char *path, int binary)
{
    char name[64];
    if (!path) {
        bdpt_ppm_name(name, (int)sizeof name, h->total_time, h->current_sample);
        path = name;
    }
    unsigned char *rgba = malloc(4 * (size_t)h->width * h->height);
    int rc = rgba ? bdpt_read_pixels(h->ctx, rgba) : BDPT_ENOMEM;
    if (rc == BDPT_OK)
        rc = binary ? bdpt_save_ppm_binary(path, rgba, h->width, h->height)
                    : bdpt_save_ppm(path, rgba, h->width, h->height);
    report(h, rc, "SavePPM");
    free(rgba);
    return rc;
}

/* --denoise: the same file from the denoised frame's pixels (bdpt_denoise) */
__attribute__((unused)) static int save_denoised_ppm(host *h, const char *path, int binary,
                                                     const bdpt_denoise_params *dn)
{
    unsigned char *rgba = malloc(4 * (size_t)h->width * h->height);
    int rc = rgba ? bdpt_denoise(h->ctx, dn, NULL, rgba) : BDPT_ENOMEM;
    if (rc == BDPT_OK)
        rc = binary ? bdpt_save_ppm_binary(path, rgba, h->width, h->height)
                    : bdpt_save_ppm(path, rgba, h->width, h->height);
    report(h, rc, "Denoised SavePPM");
    free(rgba);
    return rc;
}

/* --denoise-noise: the same file from the noise-guided filter's pixels (bdpt_denoise_noise) */
__attribute__((unused)) static int save_denoised_noise_ppm(host *h, const char *path, int binary,
                                                           const bdpt_denoise_noise_params *dn)
{
    unsigned char *rgba = malloc(4 * (size_t)h->width * h->height);
    int rc = rgba ? bdpt_denoise_noise(h->ctx, dn, NULL, rgba, NULL) : BDPT_ENOMEM;
    if (rc == BDPT_OK)
        rc = binary ? bdpt_save_ppm_binary(path, rgba, h->width, h->height)
                    : bdpt_save_ppm(path, rgba, h->width, h->height);
    report(h, rc, "Noise-guided denoised SavePPM");
    free(rgba);
    return rc;
}

/* --reproject: the same file from the preview's pixels (bdpt_reproject) */
__attribute__((unused)) static int save_preview_ppm(host *h, const char *path, int binary)
{
    unsigned char *rgba = malloc(4 * (size_t)h->width * h->height);
    int rc = rgba ? bdpt_reproject(h->ctx, &h->rp, NULL, NULL, rgba) : BDPT_ENOMEM;
    if (rc == BDPT_OK)
        rc = binary ? bdpt_save_ppm_binary(path, rgba, h->width, h->height)
                    : bdpt_save_ppm(path, rgba, h->width, h->height);
    report(h, rc, "Preview SavePPM");
    free(rgba);
    return rc;
}

/* --reproject --denoise: the same file from the denoised preview's pixels (bdpt_preview_denoise) */
__attribute__((unused)) static int save_denoised_preview_ppm(host *h, const char *path, int binary,
                                                             const bdpt_preview_params *pv)
{
    unsigned char *rgba = malloc(4 * (size_t)h->width * h->height);
    int rc = rgba ? bdpt_preview_denoise(h->ctx, pv, NULL, NULL, rgba) : BDPT_ENOMEM;
    if (rc == BDPT_OK)
        rc = binary ? bdpt_save_ppm_binary(path, rgba, h->width, h->height)
                    : bdpt_save_ppm(path, rgba, h->width, h->height);
    report(h, rc, "Denoised preview SavePPM");
    free(rgba);
    return rc;
}

/* --until E: passes in batches until the noise estimate says the frame is good enough
 * (bdpt_noise_estimate with remark after every batch: some pixel valid, none pending, no tile over
 * the threshold) or max_spp passes are rendered; one report line on stderr.  Returns 1 when
 * converged, 0 when not, -1 on an error. */
/* keep_mark (--denoise-noise): a pixel that has just re-marked has no fresh samples and so no
 * variance for bdpt_denoise_noise, so every check estimates without remark first and re-marks (a
 * second estimate) only when the loop goes on: the mark the last check used stays in place. */
__attribute__((unused)) static int render_until(host *h, const bdpt_noise_params *np, int max_spp, int batch,
                                                int keep_mark)
{
    bdpt_noise_summary s;
    int converged = 0;
    memset(&s, 0, sizeof s);
    const int first = h->current_sample;
    bdpt_noise_params look = *np;
    if (keep_mark) look.remark = 0;
    for (;;) {
        update_rendering(h, batch);
        int rc = bdpt_noise_estimate(h->ctx, &look, NULL, NULL, NULL, &s);
        report(h, rc, "Noise estimate");
        if (rc != BDPT_OK) return -1;
        converged = s.valid_pixels > 0 && s.pending_pixels == 0 && s.tiles_over == 0;
        if (converged || h->current_sample >= max_spp) break;
        if (keep_mark) {
            bdpt_noise_summary again;
            rc = bdpt_noise_estimate(h->ctx, np, NULL, NULL, NULL, &again);
            report(h, rc, "Noise re-mark");
            if (rc != BDPT_OK) return -1;
        }
    }
    fprintf(stderr, "Until %g: %d passes (%d in this render), %s, worst tile %.9g, mean %.17g\n", (double)np->threshold,
            h->current_sample, h->current_sample - first, converged ? "converged" : "not converged",
            (double)s.max_tile, s.mean);
    return converged;
}

/* --until E --adaptive: the same loop, but every 32 x 8 tile stops on its own: a batch renders only
 * the tiles not yet retired (bdpt_path_passes_tiles), and after its estimate a tile retires -- for
 * good -- when none of its pixels is pending, its error is at most the threshold (or it has no
 * valid pixel) and min_spp passes are done.  Converged when every tile is retired.  One report
 * line on stderr with the pixel-passes rendered against width x height x passes. */
__attribute__((unused)) static int render_until_adaptive(host *h, const bdpt_noise_params *np, int max_spp, int batch,
                                                         int min_spp)
{
    int tx = 0, ty = 0, converged = 0, left = 0;
    if (bdpt_noise_tiles(h->ctx, &tx, &ty) != BDPT_OK) {
        report(h, BDPT_EINVAL, "Noise tiles");
        return -1;
    }
    const int nt = tx * ty, first = h->current_sample;
    unsigned char *live = malloc((size_t)nt);
    float *err = malloc(sizeof(float) * (size_t)nt);
    unsigned *valid = malloc(sizeof(unsigned) * (size_t)nt), *pending = malloc(sizeof(unsigned) * (size_t)nt);
    bdpt_noise_summary s;
    long long pixel_passes = 0;
    int rc = live && err && valid && pending ? BDPT_OK : BDPT_ENOMEM;
    memset(&s, 0, sizeof s);
    if (rc == BDPT_OK) memset(live, 1, (size_t)nt);
    while (rc == BDPT_OK) {
        long long pixels = 0;
        for (int t = 0; t < nt; t++) {
            const int w = h->width - (t % tx) * BDPT_NOISE_TW, r = h->height - (t / tx) * BDPT_NOISE_TH;
            if (live[t]) pixels += (long long)(w < BDPT_NOISE_TW ? w : BDPT_NOISE_TW) * (r < BDPT_NOISE_TH ? r : BDPT_NOISE_TH);
        }
        const int before = h->current_sample;
        update_rendering_tiles(h, batch, live, pixels);
        pixel_passes += pixels * (h->current_sample - before);
        rc = bdpt_noise_estimate(h->ctx, np, NULL, err, valid, &s);
        if (rc == BDPT_OK) rc = bdpt_noise_tile_pending(h->ctx, pending);
        if (rc != BDPT_OK) break;
        left = 0;
        for (int t = 0; t < nt; t++) {
            if (live[t] && pending[t] == 0 && (valid[t] == 0 || err[t] <= np->threshold) && h->current_sample >= min_spp)
                live[t] = 0;
            left += live[t];
        }
        converged = left == 0;
        if (converged || h->current_sample >= max_spp) break;
    }
    report(h, rc, "Adaptive noise estimate");
    if (rc == BDPT_OK)
        fprintf(stderr, "Until %g adaptive: %d passes (%d in this render), %s, %d of %d tiles left, "
                "%lld pixel-passes of %lld (width x height x passes)\n", (double)np->threshold, h->current_sample,
                h->current_sample - first, converged ? "converged" : "not converged", left, nt, pixel_passes,
                (long long)h->width * h->height * (h->current_sample - first));
    free(live);
    free(err);
    free(valid);
    free(pending);
    return rc == BDPT_OK ? converged : -1;
}

/* what a checkpoint carries besides the frame: the pass schedule and the host counters */
typedef struct {
    bdpt_pass_state ps;
    int current_sample, reinit_counter, current_sphere;
    float total_time;
} host_state;

__attribute__((unused)) static void get_state(const host *h, host_state *s)
{
    memset(s, 0, sizeof *s);
    s->ps = h->ps;
    s->current_sample = h->current_sample;
    s->reinit_counter = h->reinit_counter;
    s->current_sphere = h->current_sphere;
    s->total_time = h->total_time;
}

static void key(host *h, int k)
{
    if (k == 'p') {
        (void)save_ppm(h, NULL, 0);
        return;
    }
    int code = k;
    if (k == 'U') code = BDPT_KEY_UP;
    else if (k == 'D') code = BDPT_KEY_DOWN;
    else if (k == 'L') code = BDPT_KEY_LEFT;
    else if (k == 'R') code = BDPT_KEY_RIGHT;
    else if (k == 'P') code = BDPT_KEY_PAGE_UP;
    else if (k == 'Q') code = BDPT_KEY_PAGE_DOWN;
    if (k == '+' || k == '-') {
        h->current_sphere = k == '+' ? (h->current_sphere + 1) % (int)h->n
                                     : (h->current_sphere + ((int)h->n - 1)) % (int)h->n;
        fprintf(stderr, "Selected sphere %d (%f %f %f)\n", h->current_sphere,
                h->spheres[h->current_sphere].p.x, h->spheres[h->current_sphere].p.y,
                h->spheres[h->current_sphere].p.z);
        reinit_scene(h);
    } else if (bdpt_sphere_key(h->spheres, h->n, h->current_sphere, k)) {
        reinit_scene(h);
    } else if (bdpt_camera_key(&h->camera, code)) {
        /* the context still holds the old camera and the frame ReInit is about to discard */
        if (h->reuse_history) report(h, bdpt_history_capture(h->ctx, &h->rp), "History capture");
        reinit(h);
    }
}

#endif
