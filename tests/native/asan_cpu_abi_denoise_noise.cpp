// asan_cpu_abi_denoise_noise.cpp -- TEST INFRASTRUCTURE: the top of the sanitizer build's HIP-free
// context layer (the Makefile's ASAN_ABI_SRC builds this file when it exists).  It is
// asan_cpu_abi_noise.cpp plus the entry point smallpt's `--denoise-noise` calls, on the product's CPU
// backend.
#include "asan_cpu_abi_noise.cpp"

extern "C" int bdpt_denoise_noise(bdpt_ctx* c, const bdpt_denoise_noise_params* p, bdpt_vec* colors_out,
                                  unsigned char* rgba_out, float* variance_out) {
    if (!c) return BDPT_EINVAL;
    if (!p || (!colors_out && !rgba_out) || p->levels < 1 || p->levels > 8 || p->normal_power < 0 ||
        p->normal_power > 6 || !(p->sigma_color > 0.f) || !(p->noise_sigma > 0.f && p->noise_sigma < INFINITY) ||
        (p->materials != BDPT_DENOISE_DIFFUSE && p->materials != BDPT_DENOISE_ALL))
        return fail(c, BDPT_EINVAL, "bdpt_denoise_noise: bad arguments");
    if (!c->cam_set) return fail(c, BDPT_ESTATE, "bdpt_denoise_noise: camera not set");
    bdpt_cpu_denoise_noise(c->cpu, p, colors_out, rgba_out, variance_out);
    return BDPT_OK;
}
