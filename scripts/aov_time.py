"""Time the first-hit feature-buffer kernel (bdpt_aov_kernel) against a one-pass path launch.

    python scripts/aov_time.py [--width 1920 --height 1080] [--reps 200] [--out profiles/aov_timing.json]

Sizes get +1 like `smallpt` (1921x1081 by default).  Per scene, in one process and one context:
  * the kernel alone: HIP events around the launch (bdpt_last_aov_ms), no read-back (no plane is
    requested), after warm-up calls; jittered rays (sid 7), as a pass would trace them;
  * both wave-tile shapes (BDPT_AOV_TILE=64: 64x1 rows, =8: 8x8 tiles), alternating call by call, so
    the default of each traversal rests on a same-session comparison;
  * the comparator: single-pass bdpt_path_passes launches of the same frame (bdpt_last_path_ms,
    the whole call on the device; and the path kernel alone from bdpt_kernel_timing).
cornell runs the brute scan (9 spheres), complex the BVH (783 spheres) and, for information, the
brute scan too.  Medians with min / max go to the JSON file.  Needs the GPU: there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import gpu_bidirectional_raytracer_amd as g  # noqa: E402

SID = 7


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "n": len(ms)}


def time_scene(name, traversals, W, H, reps, warm, device):
    cam, sp = g.read_scene(os.path.join(g.SCENE_DIR, name + ".scn"))
    g.update_camera(cam, W, H)
    out = {"scene": name, "spheres": int(len(sp)), "size": [W, H], "aov": {}}
    with g.Renderer(sp, W, H, cam, device=device) as r:
        r.light_pass(0)
        sched = g.PassScheduler()
        sched.light()
        for trav in traversals:
            r.set_traversal(trav)
            times = {"64": [], "8": []}
            for k in range(warm + reps):
                for tile in ("64", "8"):                       # alternate the two shapes
                    os.environ["BDPT_AOV_TILE"] = tile
                    r.render_aov(sid=SID, planes=())           # kernel only: nothing is read back
                    if k >= warm:
                        times[tile].append(r.last_aov_ms())
            os.environ.pop("BDPT_AOV_TILE", None)
            r.render_aov(sid=SID, planes=())
            assert device < 0 or r.last_aov_traversal == trav    # (the CPU backend always scans)
            out["aov"][trav] = {"rows_64x1": stats(times["64"]), "tiles_8x8": stats(times["8"]),
                                "default": "tiles_8x8" if trav == "bvh" else "rows_64x1"}
        # the comparator: one-pass path launches of the same frame, same context
        r.set_traversal("bvh" if "bvh" in traversals else "auto")
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
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "aov_timing.json"))
    a = ap.parse_args()
    W, H = a.width + 1, a.height + 1
    res = {"what": "bdpt_aov_kernel alone (HIP events, no read-back) vs a one-pass bdpt_path_passes launch",
           "reps": a.reps, "warmup": a.warmup,
           "scenes": [time_scene("cornell", ["brute"], W, H, a.reps, a.warmup, a.device),
                      time_scene("complex", ["bvh", "brute"], W, H, a.reps, a.warmup, a.device)]}
    for s in res["scenes"]:
        for trav, t in s["aov"].items():
            print(f"{s['scene']:8s} {trav:5s} aov rows {t['rows_64x1']['median_ms']:.4f} ms  "
                  f"tiles {t['tiles_8x8']['median_ms']:.4f} ms")
        p = s["path_one_pass"]
        print(f"{s['scene']:8s} one path pass: call {p['call']['median_ms']:.4f} ms, "
              f"path kernel {p['path_kernel']['median_ms']:.4f} ms ({p['traversal']})")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
