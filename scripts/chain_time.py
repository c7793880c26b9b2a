"""Time the chain kernel (bdpt_chain_kernel) beside the first-hit kernel and a one-pass path launch.

    python scripts/chain_time.py [--width 1920 --height 1080] [--reps 100] [--out profiles/chain_timing.json]

Sizes get +1 like `smallpt` (1921x1081 by default).  Per case, in one process and one context:
  * the kernel alone: HIP events around the launch (bdpt_last_chain_ms), no read-back (no plane is
    requested), after warm-up calls; unjittered TRANSMIT chains, as the denoisers ask for them, and
    jittered PASS chains (sid 7), as a pass would trace them;
  * both wave-tile shapes (BDPT_CHAIN_TILE=64: 64x1 rows, =8: 8x8 tiles), alternating call by call, so
    the default of each traversal rests on a same-session comparison;
  * beside it bdpt_aov_kernel (bdpt_last_aov_ms, its default tile) and single-pass bdpt_path_passes
    launches of the same frame (bdpt_last_path_ms, the whole call on the device; and the path kernel
    alone from bdpt_kernel_timing);
  * how many pixels pass how many bounces (from one read-back, outside the timing).
cornell_mirror and hall_of_mirrors run the brute scan, complex (783 spheres) the BVH.
hall_of_mirrors' own camera starts every ray outside its small scene (all misses); "hall_gap" is the
same scene from the camera of the test fixtures, which looks into the gap between the mirror balls.
Medians with min / max go to the JSON file.  Needs the GPU: there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import gpu_bidirectional_raytracer_amd as g  # noqa: E402

SID = 7
HALL_GAP = ((0.02, 0.05, -1.2), (0.0, 0.02, 0.0))       # tests/golden/make_ref_chain_golden.py HALL_CAMERA


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "n": len(ms)}


def time_case(tag, name, trav, W, H, reps, warm, device, camera=None):
    cam, sp = g.read_scene(os.path.join(g.SCENE_DIR, name + ".scn"))
    if camera is not None:
        cam.orig, cam.target = g.Vec(*camera[0]), g.Vec(*camera[1])
    g.update_camera(cam, W, H)
    out = {"case": tag, "scene": name, "spheres": int(len(sp)), "size": [W, H], "traversal": trav, "chain": {}}
    with g.Renderer(sp, W, H, cam, device=device) as r:
        r.set_traversal(trav)
        r.light_pass(0)
        sched = g.PassScheduler()
        sched.light()
        c = r.render_chain(planes=("kind", "bounces"))
        out["pixels_by_bounces"] = [int(v) for v in np.bincount(c["bounces"].ravel(), minlength=8)]
        out["pixels_by_kind"] = [int(v) for v in np.bincount(c["kind"].ravel(), minlength=4)]
        for mode, kw in (("transmit_unjittered", {}), ("pass_jittered", dict(sid=SID, branch="pass"))):
            times = {"64": [], "8": []}
            for k in range(warm + reps):
                for tile in ("64", "8"):                       # alternate the two shapes
                    os.environ["BDPT_CHAIN_TILE"] = tile
                    r.render_chain(planes=(), **kw)            # kernel only: nothing is read back
                    if k >= warm:
                        times[tile].append(r.last_chain_ms())
            os.environ.pop("BDPT_CHAIN_TILE", None)
            out["chain"][mode] = {"rows_64x1": stats(times["64"]), "tiles_8x8": stats(times["8"])}
        aov_ms = []
        for k in range(warm + reps):
            r.render_aov(sid=SID, planes=())
            if k >= warm:
                aov_ms.append(r.last_aov_ms())
        out["aov"] = stats(aov_ms)
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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "chain_timing.json"))
    a = ap.parse_args()
    W, H = a.width + 1, a.height + 1
    cases = [("cornell_mirror", "cornell_mirror", "brute", None), ("hall_of_mirrors", "hall_of_mirrors", "brute", None),
             ("hall_gap", "hall_of_mirrors", "brute", HALL_GAP), ("complex", "complex", "bvh", None)]
    res = {"what": "bdpt_chain_kernel alone (HIP events, no read-back), both wave tiles alternating, beside "
                   "bdpt_aov_kernel and a one-pass bdpt_path_passes launch of the same frame",
           "reps": a.reps, "warmup": a.warmup,
           "cases": [time_case(t, n, trav, W, H, a.reps, a.warmup, a.device, cam) for t, n, trav, cam in cases]}
    for s in res["cases"]:
        for mode, t in s["chain"].items():
            print(f"{s['case']:16s} {mode:20s} rows {t['rows_64x1']['median_ms']:.4f} ms  tiles "
                  f"{t['tiles_8x8']['median_ms']:.4f} ms")
        p = s["path_one_pass"]
        print(f"{s['case']:16s} aov {s['aov']['median_ms']:.4f} ms; one path pass: call {p['call']['median_ms']:.4f} ms, "
              f"path kernel {p['path_kernel']['median_ms']:.4f} ms ({p['traversal']}); bounces {s['pixels_by_bounces']}")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
