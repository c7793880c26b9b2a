"""Time the denoised preview's kernels (bdpt_preview_denoise) against reproject() + denoise().

    python scripts/preview_time.py [--width 1920 --height 1080] [--reps 100] [--out profiles/preview_timing.json]

Sizes get +1 like `smallpt` (1921x1081 by default).  Per scene, in one process and one context:
16 passes, a capture, the `left` key, ReInit's reset and one pass -- the state an interactive user
is in after a camera key.  Then, alternating call by call so that every figure rests on a
same-session comparison, the kernels alone between HIP events (no read-back inside the interval;
only the 8-bit pixels are asked for), defaults (4 levels, normal_power 5, sigma 0.5, count_ref 8):
  * preview_denoise with the guide record {normal, id or -1} written by bdpt_reproject_kernel (the
    default) and by bdpt_denoise_pack_kernel in a launch of its own (BDPT_PREVIEW_GUIDE=pack);
  * the yardstick: reproject() and denoise() called separately (bdpt_last_reproject_ms +
    bdpt_last_denoise_ms): two first-hit kernels and the denoiser's pack pass.
cornell runs the brute scan for its first hits (9 spheres), complex the BVH (783 spheres).  Medians
with min / max go to the JSON file.  Needs the GPU: there is no fallback.
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
    out = {"scene": name, "spheres": int(len(sp)), "size": [W, H], "guide_default": "reproject_kernel"}
    px = np.empty((H, W, 4), np.uint8)
    ppx = ctypes.c_void_p(px.ctypes.data)
    rp = g._lib.ReprojectParams(0, 64.0, 0.01)
    dn = g._lib.DenoiseParams(4, 5, 0.5, 0)
    pv = g._lib.PreviewParams(rp, 4, 5, 0.5, 8.0)
    with g.Renderer(sp, W, H, cam, device=device) as r:
        r.light_pass(0)
        sched = g.PassScheduler()
        sched.light()
        r.path_passes(*sched.next(16))
        r.history_capture()
        assert g.camera_key(cam, "left")
        g.update_camera(cam, W, H)
        r.reset_accum()
        r.set_camera(cam)
        r.path_passes(*sched.next(1))
        t = {"preview_guide_in_reproject_kernel": [], "preview_guide_by_pack_kernel": [], "reproject": [],
             "denoise": [], "reproject_plus_denoise": []}
        for k in range(warm + reps):
            os.environ.pop("BDPT_PREVIEW_GUIDE", None)
            assert g.lib.bdpt_preview_denoise(r._h, ctypes.byref(pv), None, None, ppx) == 0
            a = r.last_preview_ms()
            os.environ["BDPT_PREVIEW_GUIDE"] = "pack"
            assert g.lib.bdpt_preview_denoise(r._h, ctypes.byref(pv), None, None, ppx) == 0
            b = r.last_preview_ms()
            os.environ.pop("BDPT_PREVIEW_GUIDE", None)
            assert g.lib.bdpt_reproject(r._h, ctypes.byref(rp), None, None, ppx) == 0
            c = r.last_reproject_ms()
            assert g.lib.bdpt_denoise(r._h, ctypes.byref(dn), None, ppx) == 0
            d = r.last_denoise_ms()
            if k >= warm:
                t["preview_guide_in_reproject_kernel"].append(a)
                t["preview_guide_by_pack_kernel"].append(b)
                t["reproject"].append(c)
                t["denoise"].append(d)
                t["reproject_plus_denoise"].append(c + d)
        out.update({k: stats(v) for k, v in t.items()})
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "preview_timing.json"))
    a = ap.parse_args()
    W, H = a.width + 1, a.height + 1
    res = {"what": "bdpt_preview_denoise kernels alone (HIP events, no read-back) vs bdpt_reproject + bdpt_denoise "
                   "called separately; 16 passes of history, key left, one pass; defaults, pixels out",
           "reps": a.reps, "warmup": a.warmup,
           "scenes": [time_scene(n, W, H, a.reps, a.warmup, a.device) for n in ("cornell", "complex")]}
    for s in res["scenes"]:
        print(f"{s['scene']:8s} " + "  ".join(f"{k} {s[k]['median_ms']:.4f}" for k in
                                             ("preview_guide_in_reproject_kernel", "preview_guide_by_pack_kernel",
                                              "reproject", "denoise", "reproject_plus_denoise")) + " ms")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
