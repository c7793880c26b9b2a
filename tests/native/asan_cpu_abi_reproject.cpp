// asan_cpu_abi_reproject.cpp -- TEST INFRASTRUCTURE: the sanitizer build's HIP-free context layer
// (asan_cpu_abi_denoise.cpp, included here so that its context struct is visible) plus the history
// entry points that the C host `smallpt` calls for --reproject, on the CPU backend as libbdpt.so's
// real layer routes them for BDPT_DEVICE_CPU.  `make asan` compiles this file as asan_cpu_abi.o.
#include "asan_cpu_abi_denoise.cpp"

static int rp_check(bdpt_ctx* c, const bdpt_reproject_params* p) {
    if (!p || (p->materials != BDPT_DENOISE_DIFFUSE && p->materials != BDPT_DENOISE_ALL) || !(p->max_history > 0.f) ||
        !(p->plane_tol >= 0.f))
        return fail(c, BDPT_EINVAL, "reprojection: bad parameters");
    if (!c->cam_set) return fail(c, BDPT_ESTATE, "reprojection: camera not set");
    return BDPT_OK;
}

extern "C" int bdpt_history_capture(bdpt_ctx* c, const bdpt_reproject_params* p) {
    if (!c) return BDPT_EINVAL;
    if (int rc = rp_check(c, p)) return rc;
    bdpt_cpu_history_capture(c->cpu, p);
    return BDPT_OK;
}

extern "C" int bdpt_history_clear(bdpt_ctx* c) {
    if (!c) return BDPT_EINVAL;
    bdpt_cpu_history_clear(c->cpu);
    return BDPT_OK;
}

extern "C" int bdpt_reproject(bdpt_ctx* c, const bdpt_reproject_params* p, bdpt_vec* colors_out, float* weight_out,
                              unsigned char* rgba_out) {
    if (!c) return BDPT_EINVAL;
    if (!colors_out && !weight_out && !rgba_out) return fail(c, BDPT_EINVAL, "bdpt_reproject: no output buffer");
    if (int rc = rp_check(c, p)) return rc;
    bdpt_cpu_reproject(c->cpu, p, colors_out, weight_out, rgba_out);
    return BDPT_OK;
}
