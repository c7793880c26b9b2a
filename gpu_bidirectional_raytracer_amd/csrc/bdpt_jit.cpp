// bdpt_jit.cpp -- scene-specialised path kernels, compiled at run time with hipRTC.
//
// For scenes of <= 64 spheres (not BVH-traversed) the path kernel is recompiled with the scene folded in
// (bdpt_kernels.hip BDPT_JIT): the sphere geometry {p, rad^2} as exact hex-float literals and the
// emitter mask become compile-time constants, so a coordinate difference p - o that several
// spheres share is formed once per ray (cornell's 9 spheres have 15 distinct coordinates, not
// 27) and the scalar scene loads go away: +7 % on cornell.  The float operations are the same in
// the same order, so results are bit-identical to the precompiled kernels
// (tests/test_gpu_specialize.py).  hipRTC is opened with dlopen; when it is missing or a compile
// fails, the precompiled instance runs (bdpt_last_specialized() says which one did).  A build that
// needs scratch (register spills) at 6 waves/SIMD is rebuilt at 5.  Code objects are cached per
// context and on disk ($BDPT_JIT_CACHE, else $HOME/.cache/bdpt-jit), keyed by a hash of the
// sources, the options, the hipRTC version and the device's gfx arch; the cache directory must be
// owned by the user and closed to others (created 0700), else nothing is read from or written to
// disk.  A compile takes ~1 s.
//
// What is built -- the variants, the options, and which build follows one that costs a workgroup
// or spills -- is decided in bdpt_jit_plan.h, without a HIP call.  Here: the environment read into
// a bdpt_jit_env, hipRTC, the caches, and the loop that builds what the plan says.
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <hip/hiprtc.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>
#include <string>
#include <vector>

#include "bdpt_ctx.h"
#include "bdpt_jit_src.h"

namespace {
struct rtc_api {
    bool ok = false;
    decltype(&hiprtcCreateProgram) create = nullptr;
    decltype(&hiprtcAddNameExpression) add_name = nullptr;
    decltype(&hiprtcCompileProgram) compile = nullptr;
    decltype(&hiprtcGetLoweredName) lowered = nullptr;
    decltype(&hiprtcGetCodeSize) code_size = nullptr;
    decltype(&hiprtcGetCode) code = nullptr;
    decltype(&hiprtcGetProgramLogSize) log_size = nullptr;
    decltype(&hiprtcGetProgramLog) log = nullptr;
    decltype(&hiprtcDestroyProgram) destroy = nullptr;
    int major = 0, minor = 0;                    // hiprtcVersion (part of the cache key)
};

const rtc_api& rtc() {
    static const rtc_api api = [] {
        rtc_api r;
        const char* libs[] = {"libhiprtc.so.7", "libhiprtc.so", "/opt/rocm/lib/libhiprtc.so.7",
                              "/opt/rocm/lib/libhiprtc.so"};
        void* h = nullptr;
        for (const char* l : libs)
            if ((h = dlopen(l, RTLD_NOW | RTLD_LOCAL))) break;
        if (!h) return r;
#define BDPT_RTC_SYM(f, n) r.f = (decltype(r.f))dlsym(h, n)
        BDPT_RTC_SYM(create, "hiprtcCreateProgram");
        BDPT_RTC_SYM(add_name, "hiprtcAddNameExpression");
        BDPT_RTC_SYM(compile, "hiprtcCompileProgram");
        BDPT_RTC_SYM(lowered, "hiprtcGetLoweredName");
        BDPT_RTC_SYM(code_size, "hiprtcGetCodeSize");
        BDPT_RTC_SYM(code, "hiprtcGetCode");
        BDPT_RTC_SYM(log_size, "hiprtcGetProgramLogSize");
        BDPT_RTC_SYM(log, "hiprtcGetProgramLog");
        BDPT_RTC_SYM(destroy, "hiprtcDestroyProgram");
#undef BDPT_RTC_SYM
        auto version = (decltype(&hiprtcVersion))dlsym(h, "hiprtcVersion");
        r.ok = r.create && r.add_name && r.compile && r.lowered && r.code_size && r.code &&
               r.log_size && r.log && r.destroy && version &&
               version(&r.major, &r.minor) == HIPRTC_SUCCESS;
        return r;
    }();
    return api;
}

uint64_t fnv1a(uint64_t h, const void* p, size_t n) {
    const unsigned char* b = (const unsigned char*)p;
    for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 1099511628211ull;
    return h;
}

// The on-disk cache directory, created 0700 if missing; "" (no disk cache) unless it is a
// directory owned by this user that neither group nor others can write.
std::string jit_cache_dir() {
    std::string dir;
    if (const char* d = getenv("BDPT_JIT_CACHE")) dir = d;
    else if (const char* home = getenv("HOME")) dir = std::string(home) + "/.cache/bdpt-jit";
    else return "";
    std::string d;                                           // mkdir -p, 0700
    for (size_t i = 0; i <= dir.size(); i++) {
        if ((i == dir.size() || dir[i] == '/') && !d.empty()) mkdir(d.c_str(), 0700);
        if (i < dir.size()) d += dir[i];
    }
    struct stat st;
    if (stat(dir.c_str(), &st) != 0 || !S_ISDIR(st.st_mode) || st.st_uid != getuid() ||
        (st.st_mode & (S_IWGRP | S_IWOTH)))
        return "";
    return dir;
}

bool read_file(const std::string& path, std::vector<char>& out) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return false;
    struct stat st;
    if (fstat(fileno(f), &st) != 0 || st.st_uid != getuid() || !S_ISREG(st.st_mode)) {
        fclose(f);
        return false;
    }
    out.resize(st.st_size > 0 ? (size_t)st.st_size : 0);
    const bool ok = st.st_size > 0 && fread(out.data(), 1, out.size(), f) == out.size();
    fclose(f);
    return ok;
}

// Write to a private temporary file and rename it into place only if every byte reached it.
void write_file_atomic(const std::string& path, const std::vector<char>& data) {
    const std::string tmp = path + ".tmp." + std::to_string((long)getpid());
    FILE* f = fopen(tmp.c_str(), "wb");
    if (!f) return;
    bool ok = fwrite(data.data(), 1, data.size(), f) == data.size();
    ok = (fflush(f) == 0) && ok;
    ok = (fclose(f) == 0) && ok;
    if (ok) ok = rename(tmp.c_str(), path.c_str()) == 0;
    if (!ok) unlink(tmp.c_str());
}

// Compile (or fetch from the disk cache) and load one specialised build; nullptr on failure
// (reason in c->jit_err).
hipFunction_t jit_build(bdpt_ctx* c, const std::string& name, const std::vector<std::string>& opts) {
    const rtc_api& api = rtc();
    std::string key = name;
    for (const std::string& o : opts) key += " " + o;
    const auto it = c->jit_fns.find(key);
    if (it != c->jit_fns.end()) return it->second;

    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, c->device) != hipSuccess) {
        (void)hipGetLastError();
        snprintf(c->jit_err, sizeof c->jit_err, "hipGetDeviceProperties failed");
        return nullptr;
    }
    uint64_t h = 1469598103934665603ull;
    h = fnv1a(h, kJitMain, sizeof kJitMain);
    for (int i = 0; i < kJitNumHeaders; i++) h = fnv1a(h, kJitHeaders[i], strlen(kJitHeaders[i]));
    h = fnv1a(h, key.data(), key.size());
    const int ver[2] = {api.major, api.minor};
    h = fnv1a(h, ver, sizeof ver);
    h = fnv1a(h, prop.gcnArchName, strnlen(prop.gcnArchName, sizeof prop.gcnArchName));
    char hex[40];
    snprintf(hex, sizeof hex, "%016llx", (unsigned long long)h);
    const std::string dir = jit_cache_dir();
    const std::string path = dir.empty() ? "" : dir + "/path_" + hex + ".hsaco";
    const std::string name_path = path + ".name";
    std::vector<char> code, lowered;
    if (path.empty() || !read_file(path, code) || !read_file(name_path, lowered)) {
        hiprtcProgram prog = nullptr;
        if (api.create(&prog, kJitMain, kJitMainName, kJitNumHeaders, kJitHeaders, kJitHeaderNames) != HIPRTC_SUCCESS) {
            snprintf(c->jit_err, sizeof c->jit_err, "hiprtcCreateProgram failed");
            return nullptr;
        }
        api.add_name(prog, name.c_str());
        std::vector<const char*> o;
        for (const std::string& x : opts) o.push_back(x.c_str());
        const hiprtcResult rc = api.compile(prog, (int)o.size(), o.data());
        const char* low = nullptr;
        size_t sz = 0;
        if (rc != HIPRTC_SUCCESS || api.lowered(prog, name.c_str(), &low) != HIPRTC_SUCCESS || !low ||
            api.code_size(prog, &sz) != HIPRTC_SUCCESS || sz == 0) {
            size_t ls = 0;
            std::string log;
            if (api.log_size(prog, &ls) == HIPRTC_SUCCESS && ls > 1) {
                log.resize(ls);
                api.log(prog, &log[0]);
            }
            snprintf(c->jit_err, sizeof c->jit_err, "hipRTC compile failed: %.200s", log.c_str());
            api.destroy(&prog);
            return nullptr;
        }
        code.resize(sz);
        api.code(prog, code.data());
        lowered.assign(low, low + strlen(low) + 1);
        api.destroy(&prog);
        if (!path.empty()) {
            write_file_atomic(path, code);
            write_file_atomic(name_path, lowered);
        }
    }
    if (lowered.empty() || lowered.back() != '\0') lowered.push_back('\0');
    hipModule_t mod = nullptr;
    hipFunction_t fn = nullptr;
    if (hipModuleLoadData(&mod, code.data()) != hipSuccess ||
        hipModuleGetFunction(&fn, mod, lowered.data()) != hipSuccess) {
        if (mod) (void)hipModuleUnload(mod);
        (void)hipGetLastError();
        snprintf(c->jit_err, sizeof c->jit_err, "loading the specialised code object failed");
        return nullptr;
    }
    c->jit_mods.push_back(mod);
    c->jit_fns[key] = fn;
    return fn;
}

// Build the variant for the context's scene: attempt, build, what the build reports, verdict
// (bdpt_jit_plan.h), until a build is kept; nullptr = use the precompiled instance.
hipFunction_t jit_path_kernel_build(bdpt_ctx* c, const bdpt_jit_variant& v, const bdpt_jit_env& env) {
    const unsigned n = (unsigned)c->spheres.size();
    if (!c->specialize || n < 1 || n > 64) return nullptr;          // the emitter mask is 64 bits
    if (!rtc().ok) {
        snprintf(c->jit_err, sizeof c->jit_err, "hipRTC not found");
        return nullptr;
    }
    const bdpt_jit_scene scene = bdpt_jit_scene_of(c->spheres.data(), n, bdpt_zero_exit_safe(c->spheres.data(), n) != 0);
    const std::string name = bdpt_jit_name(v, scene);
    for (bdpt_jit_attempt a = bdpt_jit_first_attempt(v, env);;) {
        hipFunction_t fn = jit_build(c, name, bdpt_jit_options(v, scene, env, a));
        if (!fn) return nullptr;
        int static_lds = -1, scratch = 0;                   // what bdpt_jit_judge takes for a failed query
        if (hipFuncGetAttribute(&static_lds, HIP_FUNC_ATTRIBUTE_SHARED_SIZE_BYTES, fn) != hipSuccess) static_lds = -1;
        if (hipFuncGetAttribute(&scratch, HIP_FUNC_ATTRIBUTE_LOCAL_SIZE_BYTES, fn) != hipSuccess) scratch = 0;
        (void)hipGetLastError();
        const bdpt_jit_verdict j = bdpt_jit_judge(v, scene, env, a, static_lds, scratch);
        if (j.keep) {
            c->jit_err[0] = 0;
            c->jit_waves = a.waves;
            c->jit_zero_exit = scene.zero_exit;
            return fn;
        }
        a = j.next;
    }
}
}  // namespace

// The one place the build's environment is read: at every call, since tests and in-process A/Bs
// change it between calls (the two planner switches as bdpt_host.cpp reads them for the planner).
bdpt_jit_env bdpt_host::jit_env() {
    bdpt_jit_env e;
    if (const char* v = getenv("BDPT_JIT_FLAGS")) e.flags = v;
    if (const char* v = getenv("BDPT_JIT_WAVES")) { e.has_waves = true; e.waves = atoi(v); }
    if (const char* v = getenv("BDPT_JIT_FUSED_WAVES")) { e.has_fused_waves = true; e.fused_waves = atoi(v); }
    e.scratch_ok = getenv("BDPT_JIT_SCRATCH_OK") != nullptr;
    e.units = units_env();
    e.fused_max_passes = fused_max_passes();
    return e;
}

bool bdpt_host::jit_srec_enabled() { return jit_env().srec_enabled(); }

// The specialised kernel of a variant for the context's scene, compiled on first use; nullptr =
// use the precompiled instance (reason in c->jit_err).  The answer is kept per variant while the
// scene, the specialise switch and the environment stay as they are.
hipFunction_t bdpt_host::jit_path_kernel(bdpt_ctx* c, const bdpt_jit_variant& v) {
    const bdpt_jit_env env = jit_env();
    bdpt_ctx::jit_memo_t& m = c->jit_memo[v.index()];
    if (m.valid && m.env == env) {
        snprintf(c->jit_err, sizeof c->jit_err, "%s", m.err.c_str());
        if (m.fn) { c->jit_waves = m.waves; c->jit_zero_exit = m.zero_exit; }
        return m.fn;
    }
    hipFunction_t fn = jit_path_kernel_build(c, v, env);
    m.valid = true;
    m.fn = fn;
    m.waves = c->jit_waves;
    m.zero_exit = c->jit_zero_exit;
    m.env = env;
    m.err = c->jit_err;
    return fn;
}

void bdpt_host::jit_forget(bdpt_ctx* c) {               // the scene or the specialise switch changed
    for (bdpt_ctx::jit_memo_t& m : c->jit_memo) m.valid = false;
}

void bdpt_host::jit_release(bdpt_ctx* c) {
    for (hipModule_t m : c->jit_mods) (void)hipModuleUnload(m);
}
