"""Time path passes over a tile mask (bdpt_path_passes_tiles) against unmasked calls, and the
adaptive RenderUntil against the plain one.

    python scripts/tiles_time.py [--width 1920 --height 1080] [--reps 5] [--out profiles/tiles_timing.json]

Sizes get +1 like `smallpt` (1921x1081 by default).  Per scene (cornell, complex), in one process
and one context in the auto stream mode: twelve unmasked calls of 128 passes first, so that the
mode's measurement is over and a decision is kept.  Then, alternating call by call so that every
figure rests on a same-session comparison, the device time (HIP events around the call, fold
included) of 128-pass calls:
  * unmasked_auto: the variant the auto mode kept (it may be pixel pools or the in-kernel fold);
  * unmasked: the same with pools and units taken out of the decision -- the kernels a masked call
    runs (it follows the decision between fused and pass streams and two or four passes per lane);
  * all / checkerboard / one_in_eight / tiles_64: masked calls over every tile, every other tile,
    every eighth tile and 64 tiles spread over the frame.
Each with M samples/s per *rendered* pixel-pass (pixels inside the frame of the tiles listed).
Then on cornell, two fresh SmallPT of the same size: RenderUntil(0.05, batch=8) plain and adaptive
-- wall time, passes, pixel-passes -- and the RMSE of both frames (clamped to [0, 1]) against a
frame of --long passes rendered in the same session.  Medians with min / max go to the JSON file.
Needs the GPU: there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import gpu_bidirectional_raytracer_amd as g  # noqa: E402

NPASS = 128
POOLS, UNITS = 16, 32                       # BDPT_CHOICE_* (include/bdpt.h)


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "n": len(ms)}


def masks(tx, ty):
    y, x = np.mgrid[0:ty, 0:tx]
    t = y * tx + x
    few = np.zeros((ty, tx), bool)
    few.reshape(-1)[np.linspace(0, tx * ty - 1, 64).astype(int)] = True
    return {"all": np.ones((ty, tx), bool), "checkerboard": (x + y) % 2 == 0, "one_in_eight": t % 8 == 0, "tiles_64": few}


def tile_pixels(mask, W, H):
    w = np.minimum(32, W - 32 * np.arange(mask.shape[1]))
    h = np.minimum(8, H - 8 * np.arange(mask.shape[0]))
    return int((np.outer(h, w) * mask).sum())


def time_scene(name, W, H, reps, warm, device):
    cam, sp = g.read_scene(os.path.join(g.SCENE_DIR, name + ".scn"))
    g.update_camera(cam, W, H)
    out = {"scene": name, "spheres": int(len(sp)), "size": [W, H], "passes_per_call": NPASS}
    with g.Renderer(sp, W, H, cam, device=device) as r:
        r.light_pass(0)
        sched = g.PassScheduler()
        sched.light()
        for _ in range(12):
            r.path_passes(*sched.next(NPASS))
        choice = r.stream_choice
        out["choice"] = r.device_mode()["choice"]
        tx, ty = r.noise_tiles()
        ms = masks(tx, ty)
        out["tiles"] = {k: int(m.sum()) for k, m in ms.items()}
        out["pixels"] = {k: tile_pixels(m, W, H) for k, m in ms.items()}
        out["pixels"]["unmasked"] = out["pixels"]["unmasked_auto"] = W * H
        t = {k: [] for k in ["unmasked_auto", "unmasked"] + list(ms)}
        modes = {}
        for k in range(warm + reps):
            for key in t:
                r.set_stream_choice(choice if key == "unmasked_auto" else choice & ~(POOLS | UNITS))
                sid, vlp = sched.next(NPASS)
                r.path_passes(sid, vlp, tiles=ms.get(key))
                modes[key] = {"streams": r.last_streams, "features": r.last_features}
                if k >= warm:
                    t[key].append(r.last_path_ms())
        out["modes"] = modes
        for key, v in t.items():
            s = stats(v)
            s["msamples_per_s_rendered"] = out["pixels"][key] * NPASS / s["median_ms"] / 1e3
            out[key] = s
    return out


def rmse(a, b):
    d = np.clip(a, 0.0, 1.0).astype(np.float64) - np.clip(b, 0.0, 1.0).astype(np.float64)
    return float(np.sqrt((d * d).mean()))


def until(width, height, device, long_passes):
    scene = os.path.join(g.SCENE_DIR, "cornell.scn")
    out = {"scene": "cornell", "threshold": 0.05, "batch": 8, "long_passes": long_passes}
    frames = {}
    for key in ("plain", "adaptive", "plain_again", "adaptive_again"):
        app = g.SmallPT(width, height, scene, device=device)
        try:
            t0 = time.perf_counter()
            est = app.RenderUntil(0.05, batch=8, adaptive=key.startswith("adaptive"))
            dt = time.perf_counter() - t0
            frames[key] = app.colors()[0]
            out[key] = {"wall_s": dt, "passes": est["passes"], "converged": est["converged"],
                        "pixel_passes": int(est.get("pixel_passes", app.width * app.height * est["passes"]))}
        finally:
            app.FreeBuffers()
    app = g.SmallPT(width, height, scene, device=device)
    try:
        while app.current_sample < long_passes:
            app.IdleFunc(128)
        ref = app.colors()[0]
    finally:
        app.FreeBuffers()
    for key, f in frames.items():
        out[key]["rmse_vs_long"] = rmse(f, ref)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--long", type=int, default=8192)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "tiles_timing.json"))
    a = ap.parse_args()
    W, H = a.width + 1, a.height + 1
    res = {"what": "128-pass path-pass calls over tile masks against unmasked calls (device ms of the call, HIP events, "
                   "alternating in one session), and RenderUntil(0.05, batch=8) adaptive against plain on cornell",
           "reps": a.reps, "warmup": a.warmup,
           "scenes": [time_scene(n, W, H, a.reps, a.warmup, a.device) for n in ("cornell", "complex")]}
    for s in res["scenes"]:
        keys = [k for k in s if isinstance(s[k], dict) and "median_ms" in s[k]]
        print(f"{s['scene']:8s} " + "  ".join(f"{k} {s[k]['median_ms']:.3f} ms ({s[k]['msamples_per_s_rendered']:.0f} M/s)"
                                               for k in keys), flush=True)
    res["render_until"] = until(a.width, a.height, a.device, a.long)
    for k in ("plain", "adaptive", "plain_again", "adaptive_again"):
        print(k, res["render_until"][k], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
