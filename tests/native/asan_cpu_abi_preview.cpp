// asan_cpu_abi_preview.cpp -- TEST INFRASTRUCTURE: the sanitizer build's HIP-free context layer
// (asan_cpu_abi_reproject.cpp, included here with the chain of files behind it) plus the entry
// point that the C host `smallpt` calls for --reproject --denoise, on the CPU backend as
// libbdpt.so's real layer routes it for BDPT_DEVICE_CPU.  `make asan` compiles this file as
// asan_cpu_abi.o.
#include "asan_cpu_abi_reproject.cpp"

#include <math.h>

extern "C" int bdpt_preview_denoise(bdpt_ctx* c, const bdpt_preview_params* p, bdpt_vec* colors_out, float* weight_out,
                                    unsigned char* rgba_out) {
    if (!c) return BDPT_EINVAL;
    if (!colors_out && !weight_out && !rgba_out) return fail(c, BDPT_EINVAL, "bdpt_preview_denoise: no output buffer");
    if (!p || p->levels < 0 || p->levels > 8 || p->normal_power < 0 || p->normal_power > 6 || !(p->sigma_color > 0.f) ||
        !(p->count_ref > 0.f && p->count_ref < INFINITY))
        return fail(c, BDPT_EINVAL, "bdpt_preview_denoise: bad parameters");
    if (int rc = rp_check(c, &p->rp)) return rc;
    bdpt_cpu_preview_denoise(c->cpu, p, colors_out, weight_out, rgba_out);
    return BDPT_OK;
}
