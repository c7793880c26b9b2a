"""Time the denoiser's kernels (bdpt_denoise) against a one-pass path launch.

    python scripts/denoise_time.py [--width 1920 --height 1080] [--reps 100] [--out profiles/denoise_timing.json]

Sizes get +1 like `smallpt` (1921x1081 by default).  Per scene, in one process and one context
that has rendered 4 passes (so the frame carries real noise):
  * the kernels alone: HIP events around the guide (bdpt_aov_kernel), pack and level launches
    (bdpt_last_denoise_ms), no read-back inside the interval; only the 8-bit pixels are asked for;
  * 1, 2, 3 and 4 levels; a level's own time is the difference of two medians (level 0 comes with
    the guide and pack kernels), and its rate is the unique traffic of 48 B per pixel over that time;
  * the four kernel variants, alternating call by call, so the default rests on a same-session
    comparison: 8x8 wave tiles or 64x1 rows straight from L2 (BDPT_DENOISE_TILE=8 / 64), and either
    of them with steps 1 and 2 served from a 32x8 tile staged with its halo in LDS (BDPT_DENOISE_LDS=1);
  * the comparator: single-pass bdpt_path_passes launches of the same frame (bdpt_last_path_ms,
    the whole call on the device; and the path kernel alone from bdpt_kernel_timing).
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

VARIANTS = {"tiles_8x8": ("8", "0"), "rows_64x1": ("64", "0"), "lds_steps_1_2_then_tiles_8x8": ("8", "1"),
            "lds_steps_1_2_then_rows_64x1": ("64", "1")}
LEVELS = (1, 2, 3, 4)


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "n": len(ms)}


def time_scene(name, W, H, reps, warm, device):
    cam, sp = g.read_scene(os.path.join(g.SCENE_DIR, name + ".scn"))
    g.update_camera(cam, W, H)
    out = {"scene": name, "spheres": int(len(sp)), "size": [W, H], "default": "lds_steps_1_2_then_rows_64x1",
           "denoise": {}}
    px = np.empty((H, W, 4), np.uint8)
    with g.Renderer(sp, W, H, cam, device=device) as r:
        r.light_pass(0)
        sched = g.PassScheduler()
        sched.light()
        r.path_passes(*sched.next(4))
        times = {v: {L: [] for L in LEVELS} for v in VARIANTS}
        for k in range(warm + reps):
            for L in LEVELS:
                prm = g._lib.DenoiseParams(L, 5, 0.5, 0)
                for v, (tile, lds) in VARIANTS.items():       # alternate the variants
                    os.environ["BDPT_DENOISE_TILE"], os.environ["BDPT_DENOISE_LDS"] = tile, lds
                    rc = g.lib.bdpt_denoise(r._h, ctypes.byref(prm), None, ctypes.c_void_p(px.ctypes.data))
                    assert rc == 0, rc
                    if k >= warm:
                        times[v][L].append(r.last_denoise_ms())
        os.environ.pop("BDPT_DENOISE_TILE", None)
        os.environ.pop("BDPT_DENOISE_LDS", None)
        for v in VARIANTS:
            total = {L: stats(times[v][L]) for L in LEVELS}
            med = [total[L]["median_ms"] for L in LEVELS]
            per = [med[0]] + [med[i] - med[i - 1] for i in range(1, len(med))]
            out["denoise"][v] = {
                "total_by_levels": {str(L): total[L] for L in LEVELS},
                "guides_pack_level0_ms": per[0],
                "level_ms": {str(i): per[i] for i in range(1, len(per))},
                "level_unique_GBps": {str(i): 48.0 * W * H / (per[i] * 1e-3) / 1e9 for i in range(1, len(per))
                                      if per[i] > 0},
            }
        # the comparator: one-pass path launches of the same frame, same context
        call_ms, kern_ms = [], []
        for k in range(warm + reps):
            sid, vlp = sched.next(1)
            r.kernel_timing(reset=True)
            r.path_passes(sid, vlp)
            if k >= warm:
                call_ms.append(r.last_path_ms())
                kern_ms.append(r.kernel_timing()[0])
        out["path_one_pass"] = {"call": stats(call_ms), "path_kernel": stats(kern_ms),
                                "traversal": r.last_traversal, "features": r.last_features}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "denoise_timing.json"))
    a = ap.parse_args()
    W, H = a.width + 1, a.height + 1
    res = {"what": "bdpt_denoise kernels alone (HIP events, no read-back) vs a one-pass bdpt_path_passes launch; "
                   "normal_power 5, sigma_color 0.5, diffuse surfaces, pixels out",
           "reps": a.reps, "warmup": a.warmup,
           "scenes": [time_scene(n, W, H, a.reps, a.warmup, a.device) for n in ("cornell", "complex")]}
    for s in res["scenes"]:
        for v, t in s["denoise"].items():
            tot = t["total_by_levels"]
            print(f"{s['scene']:8s} {v:28s} 1..4 levels: " + "  ".join(f"{tot[str(L)]['median_ms']:.4f}" for L in LEVELS) +
                  " ms; levels 1..3 alone: " + "  ".join(f"{t['level_ms'][str(i)]:.4f}" for i in (1, 2, 3)) + " ms")
        p = s["path_one_pass"]
        print(f"{s['scene']:8s} one path pass: call {p['call']['median_ms']:.4f} ms, "
              f"path kernel {p['path_kernel']['median_ms']:.4f} ms ({p['traversal']})")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
