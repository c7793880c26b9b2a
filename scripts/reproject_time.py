"""Time the reprojection's kernels (bdpt_reproject, bdpt_history_capture) against a one-pass path
launch and a four-level denoise on the same context.

    python scripts/reproject_time.py [--width 1920 --height 1080] [--reps 100] [--out profiles/reproject_timing.json]

Sizes get +1 like `smallpt` (1921x1081 by default).  Per scene, in one process and one context: 16
passes, a capture, the camera key `left`, the reset and one pass -- the state a viewer is in right
after a camera move.  Then, medians after warm-up:
  * bdpt_reproject, kernels alone: HIP events around the first-hit kernel (bdpt_aov_kernel) and
    bdpt_reproject_kernel (bdpt_last_reproject_ms), no read-back inside the interval; only the 8-bit
    pixels are asked for.  The two wave tiles, 64x1 rows and 8x8 (BDPT_REPROJECT_TILE=64 / 8),
    alternate call by call, so the default rests on a same-session comparison;
  * the first-hit kernel alone (bdpt_last_aov_ms of a whole-frame render_aov); the gather's own
    time is the difference of the two medians, and its rate the unique traffic over that time:
    per pixel 28 B of first hit, 16 B of colour and counter, 32 B of history and 4 B of pixels out;
  * bdpt_history_capture (first hit, guide pack, gather writing the next history's records), the
    tiles alternating likewise -- each capture blends the history once more, which changes values,
    not traffic;
  * the comparators: single-pass bdpt_path_passes launches (bdpt_last_path_ms, and the path kernel
    alone from bdpt_kernel_timing) and the default four-level bdpt_denoise (bdpt_last_denoise_ms).
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

TILES = {"rows_64x1": "64", "tiles_8x8": "8"}
GATHER_BYTES = 28 + 16 + 32 + 4


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "n": len(ms)}


def time_scene(name, W, H, reps, warm, device):
    cam, sp = g.read_scene(os.path.join(g.SCENE_DIR, name + ".scn"))
    g.update_camera(cam, W, H)
    out = {"scene": name, "spheres": int(len(sp)), "size": [W, H], "default": "rows_64x1"}
    px = np.empty((H, W, 4), np.uint8)
    ppx = ctypes.c_void_p(px.ctypes.data)
    prm = g._lib.ReprojectParams(0, 64.0, 0.01)
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
        w = r.reproject(weight=True)[1]
        out["pixels_taking_history"] = float((w > 1).mean())
        rp = {t: [] for t in TILES}
        cap = {t: [] for t in TILES}
        for k in range(warm + reps):
            for t, env in TILES.items():                      # alternate the variants
                os.environ["BDPT_REPROJECT_TILE"] = env
                rc = g.lib.bdpt_reproject(r._h, ctypes.byref(prm), None, None, ppx)
                assert rc == 0, rc
                if k >= warm:
                    rp[t].append(r.last_reproject_ms())
        aov = []
        for k in range(warm + reps):
            buf = g._lib.AovBuffers()
            ids = np.empty((H, W), np.int32)
            buf.id = ids.ctypes.data
            rc = g.lib.bdpt_render_aov(r._h, 0, 0, W, H, 0, 0, ctypes.byref(buf))
            assert rc == 0, rc
            if k >= warm:
                aov.append(r.last_aov_ms())
        for k in range(warm + reps):
            for t, env in TILES.items():
                os.environ["BDPT_REPROJECT_TILE"] = env
                rc = g.lib.bdpt_history_capture(r._h, ctypes.byref(prm))
                assert rc == 0, rc
                if k >= warm:
                    cap[t].append(r.last_reproject_ms())
        os.environ.pop("BDPT_REPROJECT_TILE", None)
        out["first_hit_kernel"] = stats(aov)
        out["reproject"], out["capture"] = {}, {}
        for t in TILES:
            s = stats(rp[t])
            own = s["median_ms"] - out["first_hit_kernel"]["median_ms"]
            s["gather_alone_ms"] = own
            if own > 0:
                s["gather_unique_GBps"] = GATHER_BYTES * W * H / (own * 1e-3) / 1e9
            out["reproject"][t] = s
            out["capture"][t] = stats(cap[t])
        dn = []
        dprm = g._lib.DenoiseParams(4, 5, 0.5, 0)
        for k in range(warm + reps):
            rc = g.lib.bdpt_denoise(r._h, ctypes.byref(dprm), None, ppx)
            assert rc == 0, rc
            if k >= warm:
                dn.append(r.last_denoise_ms())
        out["denoise_four_levels"] = stats(dn)
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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "reproject_timing.json"))
    a = ap.parse_args()
    W, H = a.width + 1, a.height + 1
    res = {"what": "bdpt_reproject / bdpt_history_capture kernels alone (HIP events, no read-back) vs a one-pass "
                   "bdpt_path_passes launch and a four-level bdpt_denoise; 16 passes of history, key `left`, one pass; "
                   "defaults (diffuse, max_history 64, plane_tol 0.01), pixels out",
           "reps": a.reps, "warmup": a.warmup,
           "scenes": [time_scene(n, W, H, a.reps, a.warmup, a.device) for n in ("cornell", "complex")]}
    for s in res["scenes"]:
        for t in TILES:
            rp, cp = s["reproject"][t], s["capture"][t]
            print(f"{s['scene']:8s} {t:10s} reproject {rp['median_ms']:.4f} ms (gather alone {rp['gather_alone_ms']:.4f}), "
                  f"capture {cp['median_ms']:.4f} ms")
        p = s["path_one_pass"]
        print(f"{s['scene']:8s} first hit {s['first_hit_kernel']['median_ms']:.4f} ms, denoise x4 "
              f"{s['denoise_four_levels']['median_ms']:.4f} ms, one path pass: call {p['call']['median_ms']:.4f} ms, "
              f"path kernel {p['path_kernel']['median_ms']:.4f} ms ({p['traversal']}); "
              f"{100 * s['pixels_taking_history']:.0f} % of the pixels take history")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
