// asan_cpu_abi_noise.cpp -- TEST INFRASTRUCTURE: the top of the sanitizer build's HIP-free context
// layer (the Makefile's ASAN_ABI_SRC builds this file when it exists).  It is asan_cpu_abi.cpp plus
// the two entry points smallpt's `--until E --adaptive` calls besides: path passes over a tile mask
// and the last estimate's pending counts per tile, both on the product's CPU backend.
#include "asan_cpu_abi.cpp"

extern "C" int bdpt_path_passes_tiles(bdpt_ctx* c, const unsigned* sid, const int* vlp, int npass,
                                      const unsigned char* tile_mask) {
    if (!tile_mask) return bdpt_path_passes(c, sid, vlp, npass);
    if (!c->rand_ready || !c->cam_set) return fail(c, BDPT_ESTATE, "light pass / camera missing");
    bdpt_cpu_path_passes(c->cpu, sid, vlp, npass, tile_mask);
    return BDPT_OK;
}

extern "C" int bdpt_noise_tile_pending(bdpt_ctx* c, unsigned* tile_pending) {
    if (!tile_pending) return fail(c, BDPT_EINVAL, "bdpt_noise_tile_pending: no output buffer");
    if (!bdpt_cpu_noise_tile_pending(c->cpu, tile_pending)) return fail(c, BDPT_ESTATE, "bdpt_noise_tile_pending: no estimate made");
    return BDPT_OK;
}
