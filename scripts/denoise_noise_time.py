"""Time the noise-guided denoiser's kernels (bdpt_denoise_noise) next to the plain denoiser's.

    python scripts/denoise_noise_time.py [--width 1920 --height 1080] [--reps 100]
                                         [--out profiles/denoise_noise_timing.json]

Sizes get +1 like `smallpt` (1921x1081 by default).  Per scene, in one process and one context that
has rendered 8 passes with a mark after 4 (so every pixel has a variance estimate and the frame
carries real noise), the defaults of both filters (4 levels, normal_power 5, diffuse surfaces), only
the 8-bit pixels asked for:
  * the kernels alone: HIP events around the guide, pack, (prefilter) and level launches
    (bdpt_last_denoise_ms / bdpt_last_denoise_noise_ms), no read-back inside the interval;
  * three calls alternate call by call, so the ratios rest on a same-session comparison: bdpt_denoise,
    bdpt_denoise_noise, and bdpt_denoise_noise with its prefilter left out (BDPT_DNOISE_PREFILTER=0, an
    experiment switch: the result is then not the definition's), whose difference to the full call
    is the prefilter's own time;
  * the ratio of the new call to bdpt_denoise and the prefilter's share of the new call.
cornell runs the brute scan for its guides (9 spheres), complex the BVH (783 spheres).  Medians with
min / max go to the JSON file.  Needs the GPU: there is no fallback.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import gpu_bidirectional_raytracer_amd as g  # noqa: E402


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "n": len(ms)}


def time_scene(name, W, H, reps, warm, device):
    cam, sp = g.read_scene(os.path.join(g.SCENE_DIR, name + ".scn"))
    g.update_camera(cam, W, H)
    out = {"scene": name, "spheres": int(len(sp)), "size": [W, H]}
    px = np.empty((H, W, 4), np.uint8)
    ptr = ctypes.c_void_p(px.ctypes.data)
    with g.Renderer(sp, W, H, cam, device=device) as r:
        r.light_pass(0)
        sched = g.PassScheduler()
        sched.light()
        r.path_passes(*sched.next(4))
        r.noise_mark()
        r.path_passes(*sched.next(4))
        plain = g._lib.DenoiseParams(4, 5, 0.5, 0)
        noise = g._lib.DenoiseNoiseParams(4, 5, 0.5, 0, 1.0)
        times = {"denoise": [], "denoise_noise": [], "denoise_noise_without_prefilter": []}
        for k in range(warm + reps):
            assert g.lib.bdpt_denoise(r._h, ctypes.byref(plain), None, ptr) == 0
            a = r.last_denoise_ms()
            assert g.lib.bdpt_denoise_noise(r._h, ctypes.byref(noise), None, ptr, None) == 0
            b = r.last_denoise_noise_ms()
            os.environ["BDPT_DNOISE_PREFILTER"] = "0"
            try:
                assert g.lib.bdpt_denoise_noise(r._h, ctypes.byref(noise), None, ptr, None) == 0
            finally:
                os.environ.pop("BDPT_DNOISE_PREFILTER", None)
            c = r.last_denoise_noise_ms()
            if k >= warm:
                for key, ms in zip(times, (a, b, c)):
                    times[key].append(ms)
        var = r.denoise_noise(variance=True)[1]
        out["pixels_with_a_variance"] = int((var >= 0).sum())
    out.update({key: stats(ms) for key, ms in times.items()})
    full, without = out["denoise_noise"]["median_ms"], out["denoise_noise_without_prefilter"]["median_ms"]
    out["ratio_to_denoise"] = full / out["denoise"]["median_ms"]
    out["prefilter_ms"] = full - without
    out["prefilter_share"] = (full - without) / full
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "denoise_noise_timing.json"))
    a = ap.parse_args()
    W, H = a.width + 1, a.height + 1
    res = {"what": "bdpt_denoise_noise kernels alone (HIP events, no read-back) next to bdpt_denoise's, alternating call "
                   "by call; 4 levels, normal_power 5, sigma_color 0.5, noise_sigma 1, diffuse surfaces, pixels out; "
                   "8 passes with the mark after 4",
           "reps": a.reps, "warmup": a.warmup,
           "scenes": [time_scene(n, W, H, a.reps, a.warmup, a.device) for n in ("cornell", "complex")]}
    for s in res["scenes"]:
        print(f"{s['scene']:8s} denoise {s['denoise']['median_ms']:.4f} ms, denoise_noise {s['denoise_noise']['median_ms']:.4f} ms "
              f"(x{s['ratio_to_denoise']:.3f}), prefilter {s['prefilter_ms']:.4f} ms ({100 * s['prefilter_share']:.1f} %)")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
