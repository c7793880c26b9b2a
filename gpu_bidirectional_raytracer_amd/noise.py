"""Render a scene until it is good enough, and write the noise estimate, from the command line:

    python -m gpu_bidirectional_raytracer_amd.noise <width> <height> <scene> --out PREFIX
                                  [--until E] [--max-spp N] [--batch B] [--device D] [--ppm]
                                  [--adaptive [--min-spp N]] [--denoise [--noise-sigma S]]

Sizes get +1 like `smallpt` (smallpt_cpu.c:409-410).  SmallPT.RenderUntil: batches of B passes
(default 8), after each a noise estimate with re-marking (Renderer.noise_estimate), until some pixel
is valid, none is pending and no 32 x 8 tile's error is over E (default 0.05), or until N passes
(default 4096) are rendered.  Writes PREFIX.npz with the last estimate: error [H, W] float32 (-1
where not valid; row 0 is the frame's bottom row, as in read_radiance), tile_error and tile_valid
[tiles_y, tiles_x], and summary, one record with the fields of bdpt_noise_summary plus threshold,
passes and converged.  --ppm also writes PREFIX_error.ppm, a grey heat map through save_ppm
(bottom-up rows, as SavePPM): black is no error or not valid, white is 2 E or more.
--adaptive stops every 32 x 8 tile on its own (RenderUntil(adaptive=True, min_passes=N): a tile is
not rendered again once none of its pixels is pending and its error is at most E); the archive then
also holds retired_at and retired_error [tiles_y, tiles_x], pixel_passes, and counter [H, W], the
passes every pixel got.
--denoise (not with --adaptive) also filters the frame the loop stops at with the noise-guided
denoiser (RenderUntil(denoise=True, noise_sigma=S), default S = 1: the mark the last check used is
still in place) and adds denoised [H, W, 3] float32 and variance [H, W] float32 (-1 where there is
none) to the archive.
"""
from __future__ import annotations

import argparse
import sys

import numpy as np

from . import SmallPT, save_ppm

SUMMARY_DTYPE = np.dtype([("valid_pixels", np.int64), ("pending_pixels", np.int64), ("tiles_x", np.int32),
                          ("tiles_y", np.int32), ("valid_tiles", np.int32), ("tiles_over", np.int32),
                          ("mean", np.float64), ("max_tile", np.float32), ("threshold", np.float32),
                          ("passes", np.int32), ("converged", np.bool_)])


def summary_record(est: dict, threshold: float) -> np.ndarray:
    """The scalar fields of a RenderUntil result as one SUMMARY_DTYPE record."""
    rec = np.zeros((), SUMMARY_DTYPE)
    for name in SUMMARY_DTYPE.names:
        rec[name] = threshold if name == "threshold" else est[name]
    return rec


def error_rgba(error: np.ndarray, threshold: float) -> np.ndarray:
    """The per-pixel plane as 8-bit grey: 0 for no error or an invalid pixel, 255 from 2 x threshold."""
    full = 2.0 * threshold if threshold > 0 else 1.0
    with np.errstate(invalid="ignore"):
        g = np.clip(np.rint(np.clip(np.nan_to_num(error.astype(np.float64), nan=0.0), 0.0, None) / full * 255.0), 0, 255)
    g = g.astype(np.uint8)
    return np.stack([g, g, g, np.zeros_like(g)], axis=2)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m gpu_bidirectional_raytracer_amd.noise", description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("width", type=int)
    ap.add_argument("height", type=int)
    ap.add_argument("scene")
    ap.add_argument("--out", required=True, metavar="PREFIX")
    ap.add_argument("--until", type=float, default=0.05, metavar="E", help="tile error to stop at (default 0.05)")
    ap.add_argument("--max-spp", type=int, default=4096, metavar="N", help="passes to stop at anyway (default 4096)")
    ap.add_argument("--batch", type=int, default=8, metavar="B", help="passes between two checks (default 8)")
    ap.add_argument("--device", type=int, default=0, help="HIP ordinal, -1 = the CPU backend")
    ap.add_argument("--ppm", action="store_true", help="also write PREFIX_error.ppm, a grey heat map")
    ap.add_argument("--adaptive", action="store_true", help="stop every 32 x 8 tile on its own")
    ap.add_argument("--min-spp", type=int, default=0, metavar="N", help="--adaptive: no tile stops before N passes")
    ap.add_argument("--denoise", action="store_true", help="also write the noise-guided denoiser's frame and variance")
    ap.add_argument("--noise-sigma", type=float, default=1.0, metavar="S", help="--denoise: noise_sigma (default 1)")
    args = ap.parse_args(argv)
    if args.denoise and args.adaptive:
        ap.error("--denoise does not go with --adaptive")

    app = SmallPT(args.width, args.height, args.scene, device=args.device)
    try:
        est = app.RenderUntil(args.until, max_passes=args.max_spp, batch=args.batch, pixels=True,
                              adaptive=args.adaptive, min_passes=args.min_spp,
                              **(dict(denoise=True, noise_sigma=args.noise_sigma) if args.denoise else {}))
        counter = app.colors()[1] if args.adaptive else None
    finally:
        app.FreeBuffers()
    extra = {}
    if args.adaptive:
        extra = dict(retired_at=est["retired_at"], retired_error=est["retired_error"],
                     pixel_passes=np.int64(est["pixel_passes"]), counter=counter)
    if args.denoise:
        extra = dict(denoised=est["denoised"], variance=est["denoised_variance"])
    np.savez_compressed(args.out + ".npz", error=est["error"], tile_error=est["tile_error"],
                        tile_valid=est["tile_valid"], summary=summary_record(est, args.until), **extra)
    if args.ppm:
        save_ppm(args.out + "_error.ppm", error_rgba(est["error"], args.until))
    print(f"{app.width}x{app.height}: {est['passes']} passes, {'converged' if est['converged'] else 'not converged'}, "
          f"worst tile {est['max_tile']:.9g}, mean {est['mean']:.17g} -> {args.out}.npz", file=sys.stderr)
    if args.adaptive:
        print(f"adaptive: {est['pixel_passes']} pixel-passes of {app.width * app.height * est['passes']} "
              f"(width x height x passes)", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
