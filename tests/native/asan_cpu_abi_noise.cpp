// asan_cpu_abi_noise.cpp -- TEST INFRASTRUCTURE: the sanitizer build's HIP-free context layer
// (asan_cpu_abi_preview.cpp, included here with the chain of files behind it) plus the entry points
// that the C host `smallpt` calls for --until, on the CPU backend as libbdpt.so's real layer routes
// them for BDPT_DEVICE_CPU.  The calls that clear the mark (bdpt_reset_accum, bdpt_set_scene,
// bdpt_set_camera, bdpt_write_radiance) do so inside the CPU backend, so the chain's versions of
// them need no change.  `make asan` compiles this file as asan_cpu_abi.o.
#include "asan_cpu_abi_preview.cpp"

extern "C" int bdpt_noise_mark(bdpt_ctx* c) {
    if (!c) return BDPT_EINVAL;
    bdpt_cpu_noise_mark(c->cpu);
    return BDPT_OK;
}

extern "C" int bdpt_noise_clear(bdpt_ctx* c) {
    if (!c) return BDPT_EINVAL;
    bdpt_cpu_noise_clear(c->cpu);
    return BDPT_OK;
}

extern "C" int bdpt_noise_tiles(const bdpt_ctx* c, int* tiles_x, int* tiles_y) {
    if (!c) return BDPT_EINVAL;
    if (tiles_x) *tiles_x = (c->W + BDPT_NOISE_TW - 1) / BDPT_NOISE_TW;
    if (tiles_y) *tiles_y = (c->H + BDPT_NOISE_TH - 1) / BDPT_NOISE_TH;
    return BDPT_OK;
}

extern "C" int bdpt_noise_estimate(bdpt_ctx* c, const bdpt_noise_params* p, float* error_out, float* tile_error,
                                   unsigned* tile_valid, bdpt_noise_summary* summary) {
    if (!c) return BDPT_EINVAL;
    if (!p || !(p->dark > 0.f) || !(p->threshold >= 0.f)) return fail(c, BDPT_EINVAL, "bdpt_noise_estimate: bad parameters");
    if (!error_out && !tile_error && !tile_valid && !summary)
        return fail(c, BDPT_EINVAL, "bdpt_noise_estimate: no output buffer");
    int tx = 0, ty = 0;
    bdpt_noise_tiles(c, &tx, &ty);
    const size_t nt = (size_t)tx * ty;
    std::vector<float> S(nt), E(nt);
    std::vector<unsigned> cv(nt), pend(nt);
    bdpt_cpu_noise_estimate(c->cpu, p, error_out, S.data(), E.data(), cv.data(), pend.data());
    if (tile_error) memcpy(tile_error, E.data(), sizeof(float) * nt);
    if (tile_valid) memcpy(tile_valid, cv.data(), sizeof(unsigned) * nt);
    if (summary) bdpt_noise_summarize(S.data(), E.data(), cv.data(), pend.data(), tx, ty, p->threshold, summary);
    return BDPT_OK;
}
