"""Time the noise estimate's kernel (bdpt_noise_estimate) and the cost of one RenderUntil check.

    python scripts/noise_time.py [--width 1920 --height 1080] [--reps 100] [--out profiles/noise_timing.json]

Sizes get +1 like `smallpt` (1921x1081 by default).  Per scene, in one process and one context:
8 passes, a mark and a history capture, 8 more passes -- every pixel valid, a history under the same
camera so that bdpt_reproject does its full work.  Then, alternating call by call so that every
figure rests on a same-session comparison, the kernels alone between HIP events (no read-back inside
the interval):
  * estimate: tiles and summary only (what RenderUntil asks for), the mark only read;
  * estimate_pixels: the same with the per-pixel plane stored;
  * estimate_remark_all: after noise_clear, with remark, so that every pixel stores its 16-byte
    record -- the most a call can write;
  * reproject: bdpt_reproject's kernels (first hit + reprojection), pixels out: the yardstick.
Then the check as RenderUntil pays it, wall clock around the Python calls: path_passes of 8 passes
(synchronised) against noise_estimate(remark=True) (kernel, synchronise, tile read-back, summary).
Medians with min / max go to the JSON file.  Needs the GPU: there is no fallback.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

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
    ppx = ctypes.c_void_p(px.ctypes.data)
    rp = g._lib.ReprojectParams(0, 64.0, 0.01)
    with g.Renderer(sp, W, H, cam, device=device) as r:
        r.light_pass(0)
        sched = g.PassScheduler()
        sched.light()
        r.path_passes(*sched.next(8))
        r.noise_mark()
        r.history_capture()
        r.path_passes(*sched.next(8))
        mark = r.noise_read_mark()
        first = r.noise_estimate()
        assert first["valid_pixels"] == W * H
        out["estimate_at_16_passes"] = {k: first[k] for k in ("mean", "max_tile", "tiles_over", "tiles_x", "tiles_y")}
        t = {"estimate": [], "estimate_pixels": [], "estimate_remark_all": [], "reproject": []}
        for k in range(warm + reps):
            r.noise_estimate()
            a = r.last_noise_ms()
            r.noise_estimate(pixels=True)
            b = r.last_noise_ms()
            r.noise_clear()
            r.noise_estimate(remark=True)
            c = r.last_noise_ms()
            r.noise_write_mark(*mark)
            assert g.lib.bdpt_reproject(r._h, ctypes.byref(rp), None, None, ppx) == 0
            d = r.last_reproject_ms()
            if k >= warm:
                for key, v in zip(t, (a, b, c, d)):
                    t[key].append(v)
        out.update({k: stats(v) for k, v in t.items()})
        w = {"passes_8_wall": [], "check_wall": [], "check_kernel": []}
        for k in range(warm + max(reps // 4, 5)):
            sid, vlp = sched.next(8)
            t0 = time.perf_counter()
            r.path_passes(sid, vlp)
            t1 = time.perf_counter()
            r.noise_estimate(remark=True)
            t2 = time.perf_counter()
            if k >= warm:
                w["passes_8_wall"].append((t1 - t0) * 1e3)
                w["check_wall"].append((t2 - t1) * 1e3)
                w["check_kernel"].append(r.last_noise_ms())
        out.update({k: stats(v) for k, v in w.items()})
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "noise_timing.json"))
    a = ap.parse_args()
    W, H = a.width + 1, a.height + 1
    res = {"what": "bdpt_noise_kernel alone (HIP events, no read-back) against bdpt_reproject's kernels in the same "
                   "session; then one RenderUntil check (wall clock) against the 8 passes between checks",
           "reps": a.reps, "warmup": a.warmup,
           "scenes": [time_scene(n, W, H, a.reps, a.warmup, a.device) for n in ("cornell", "complex")]}
    keys = ("estimate", "estimate_pixels", "estimate_remark_all", "reproject", "passes_8_wall", "check_wall", "check_kernel")
    for s in res["scenes"]:
        print(f"{s['scene']:8s} " + "  ".join(f"{k} {s[k]['median_ms']:.4f}" for k in keys) + " ms", flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
