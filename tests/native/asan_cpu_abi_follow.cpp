// asan_cpu_abi_follow.cpp -- TEST INFRASTRUCTURE: the top of the sanitizer build's HIP-free context
// layer (the Makefile's ASAN_ABI_SRC builds this file when it exists).  It is
// asan_cpu_abi_denoise_noise.cpp plus the entry points smallpt's `--reproject-follow` calls, on the
// product's CPU backend, which keeps the switch itself.
#include "asan_cpu_abi_denoise_noise.cpp"

extern "C" int bdpt_history_follow(bdpt_ctx* c, int on) {
    if (!c) return BDPT_EINVAL;
    bdpt_cpu_history_follow(c->cpu, on);
    return BDPT_OK;
}

extern "C" int bdpt_history_motion(const bdpt_ctx* c, int* state, bdpt_vec* delta, unsigned n) {
    if (!c || (delta && n != c->spheres.size())) return BDPT_EINVAL;
    const int s = bdpt_cpu_history_motion(c->cpu, delta);
    if (state) *state = s;
    return BDPT_OK;
}
