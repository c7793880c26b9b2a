"""First-hit feature buffers of a scene from the command line:

    python -m gpu_bidirectional_raytracer_amd.aov <width> <height> <scene> --out PREFIX
                                                  [--sid N] [--device D] [--ppm] [--through]

Sizes get +1 like `smallpt` (smallpt_cpu.c:409-410).  Writes PREFIX.npz with the six arrays of
Renderer.render_aov (id, t, dp, position, normal, dir; row 0 is the frame's bottom row, as in
read_radiance).  Without --sid the rays go through the pixel centres' unjittered positions; with
--sid N they carry the jitter of a pass with that sid on the random table of the first light pass
(seed 0).  --ppm also writes PREFIX_normal.ppm and PREFIX_id.ppm through save_ppm (bottom-up rows,
as SavePPM).  No light pass and no path pass is rendered: checking a camera costs one cheap kernel.
--through adds the chain planes of Renderer.render_chain -- what every pixel shows through mirrors
and glass, glass transmitting -- to the .npz as chain_id, chain_first_id, ... chain_throughput, and
with --ppm also writes PREFIX_through_normal.ppm, the end vertices' normals.
"""
from __future__ import annotations

import argparse
import sys

import numpy as np

from . import Renderer, read_scene, save_ppm, update_camera


def normal_rgba(aov: dict) -> np.ndarray:
    """(normal + 1) / 2 as 8-bit colours, black where nothing was hit."""
    rgb = np.clip(np.rint((aov["normal"] * 0.5 + 0.5) * 255.0), 0, 255).astype(np.uint8)
    rgb[aov["id"] < 0] = 0
    return np.concatenate([rgb, np.zeros(rgb.shape[:2] + (1,), np.uint8)], axis=2)


def id_rgba(aov: dict) -> np.ndarray:
    """One fixed colour per sphere index (a multiplicative hash), black where nothing was hit."""
    sid = aov["id"].astype(np.int64)
    k = (sid + 1) * 2654435761 % 2 ** 32
    rgb = np.stack([64 + (k >> 24) % 192, 64 + (k >> 16) % 192, 64 + (k >> 8) % 192], axis=2).astype(np.uint8)
    rgb[sid < 0] = 0
    return np.concatenate([rgb, np.zeros(rgb.shape[:2] + (1,), np.uint8)], axis=2)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m gpu_bidirectional_raytracer_amd.aov", description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("width", type=int)
    ap.add_argument("height", type=int)
    ap.add_argument("scene")
    ap.add_argument("--out", required=True, metavar="PREFIX")
    ap.add_argument("--sid", type=int, default=None, help="jitter of a pass with this sid (default: none)")
    ap.add_argument("--device", type=int, default=0, help="HIP ordinal, -1 = the CPU backend")
    ap.add_argument("--ppm", action="store_true", help="also write PREFIX_normal.ppm and PREFIX_id.ppm")
    ap.add_argument("--through", action="store_true", help="add the chain planes (through mirrors and glass)")
    args = ap.parse_args(argv)

    W, H = args.width + 1, args.height + 1
    cam, spheres = read_scene(args.scene)
    update_camera(cam, W, H)
    with Renderer(spheres, W, H, cam, device=args.device) as r:
        if args.sid is not None:
            r.generate_rand(0)
        aov = r.render_aov(sid=args.sid)
        chain = r.render_chain(sid=args.sid) if args.through else {}
    np.savez_compressed(args.out + ".npz", **aov, **{f"chain_{k}": v for k, v in chain.items()})
    if args.ppm:
        save_ppm(args.out + "_normal.ppm", normal_rgba(aov))
        save_ppm(args.out + "_id.ppm", id_rgba(aov))
        if args.through:
            save_ppm(args.out + "_through_normal.ppm", normal_rgba(chain))
    hit = aov["id"] >= 0
    print(f"{W}x{H}: {int(hit.sum())} of {hit.size} pixels hit {len(np.unique(aov['id'][hit]))} of "
          f"{len(spheres)} spheres -> {args.out}.npz", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
