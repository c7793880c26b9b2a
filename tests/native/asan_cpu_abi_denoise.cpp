// asan_cpu_abi_denoise.cpp -- TEST INFRASTRUCTURE: the sanitizer build's HIP-free context layer
// (asan_cpu_abi.cpp, included here so that its context struct is visible) plus the denoiser entry
// point that the C host `smallpt` calls for --denoise, on the CPU backend as libbdpt.so's real
// layer routes it for BDPT_DEVICE_CPU.  `make asan` compiles this file as asan_cpu_abi.o.
#include "asan_cpu_abi.cpp"

extern "C" int bdpt_denoise(bdpt_ctx* c, const bdpt_denoise_params* p, bdpt_vec* colors_out,
                            unsigned char* rgba_out) {
    if (!c) return BDPT_EINVAL;
    if (!p || (!colors_out && !rgba_out) || p->levels < 1 || p->levels > 8 || p->normal_power < 0 ||
        p->normal_power > 6 || !(p->sigma_color > 0.f) ||
        (p->materials != BDPT_DENOISE_DIFFUSE && p->materials != BDPT_DENOISE_ALL))
        return fail(c, BDPT_EINVAL, "bdpt_denoise: bad arguments");
    if (!c->cam_set) return fail(c, BDPT_ESTATE, "bdpt_denoise: camera not set");
    bdpt_cpu_denoise(c->cpu, p, colors_out, rgba_out);
    return BDPT_OK;
}
