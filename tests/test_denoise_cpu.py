"""The edge-avoiding wavelet denoiser (include/bdpt.h bdpt_denoise) on the CPU backend
(device = BDPT_DEVICE_CPU, csrc/bdpt_cpu.cpp bdpt_cpu_denoise); runs without a GPU.

The definition is stated once more in numpy float32 (tests/denoise_common.py np_denoise) and the
backend must reproduce it bit for bit: rendered 4-pass frames of four scenes over the parameter
sweep, synthetic radiance with zeros, denormal-range and huge values, pass-through of ineligible
pixels, the 8-bit pixels, the error codes, side effects, the command line, and the one test with a
tolerance -- that the filter actually removes noise (RMSE against a 260-pass frame)."""
import os
import subprocess

import numpy as np
import pytest

import gpu_bidirectional_raytracer_amd as g
from aov_common import bits, same, scene, schedule
from conftest import REPO, SCENES
from denoise_common import (DEFAULTS, FRAMES, SWEEP, assert_errors, assert_non_interference, eligible, np_denoise,
                            rendered_frame, synthetic_radiance, to_rgba)

CPU = -1


@pytest.fixture(autouse=True)
def threads(monkeypatch):
    monkeypatch.setenv("BDPT_CPU_THREADS", "4")


@pytest.mark.parametrize("name,W,H", FRAMES)
def test_cpu_backend_equals_the_numpy_definition(name, W, H):
    cam, sp, col, cnt = rendered_frame(CPU, name, W, H)
    assert (cnt == 4).all() and np.isfinite(col).all()
    with g.Renderer(sp, W, H, cam, device=CPU) as r:
        r.write_radiance(col, cnt)
        aov = r.render_aov()
        changed = 0
        for prm in SWEEP:
            out = r.denoise(**prm)
            same(out, np_denoise(col, aov["id"], aov["normal"], sp["refl"], **prm), f"{name} {W}x{H} {prm}")
            el = eligible(aov["id"], sp["refl"], prm["materials"])
            same(out[~el], col[~el], f"{name} {prm}: ineligible pixels are the input")
            changed += int((bits(out) != bits(col)).any(axis=-1).sum())
        same(r.read_radiance()[0], col, "the accumulation is only read")
    assert changed > 0
    seen = set(np.unique(sp["refl"][aov["id"][aov["id"] >= 0]]).tolist())   # the materials the frame shows
    if name == "cornell_glass":
        assert {g.DIFF, g.REFR, g.LITE} <= seen
    if (name, W) == ("cornell", 33):
        assert {g.DIFF, g.SPEC, g.REFR, g.LITE} <= seen
    if name in ("caustic", "complex"):
        assert (aov["id"] < 0).any()


def test_small_frame_with_every_later_tap_outside():
    """7x5, levels = 3 .. 8: from step 8 on a level's off-centre taps are all outside the frame, so it
    returns its input -- eligible pixels as sc * (1 / sw) with the centre's weight alone."""
    cam, sp, col, cnt = rendered_frame(CPU, "cornell", 7, 5)
    with g.Renderer(sp, 7, 5, cam, device=CPU) as r:
        r.write_radiance(col, cnt)
        aov = r.render_aov()
        for levels in (3, 4, 8):
            prm = dict(DEFAULTS, levels=levels)
            same(r.denoise(**prm), np_denoise(col, aov["id"], aov["normal"], sp["refl"], **prm), f"levels {levels}")


@pytest.mark.parametrize("materials", ["diffuse", "all"])
def test_synthetic_radiance_with_underflowing_weights(materials):
    """sigma_color = 1e-3: 1 / (1 + e2 * 1e6 * 4^k) runs from 1 (equal neighbours) through the
    denormal range to 1 / inf = 0 (1e18 against anything); normal_power 6 takes the cosine to its
    64th power, which underflows on the small spheres."""
    name, W, H = "cornell_glass", 40, 33
    cam, sp = scene(name, W, H)
    col = synthetic_radiance(W, H)
    with g.Renderer(sp, W, H, cam, device=CPU) as r:
        r.write_radiance(col, np.full((H, W), 3, np.uint32))
        aov = r.render_aov()
        for levels, npow in ((1, 6), (4, 6), (5, 5), (2, 0)):
            prm = dict(levels=levels, normal_power=npow, sigma_color=1e-3, materials=materials)
            out = r.denoise(**prm)
            same(out, np_denoise(col, aov["id"], aov["normal"], sp["refl"], **prm), f"synthetic {prm}")
            same(r.denoise(**prm), out, "a second call")
            assert np.isfinite(out).all()
    el = eligible(aov["id"], sp["refl"], materials)
    same(out[~el], col[~el], "ineligible pixels are the input")
    assert el.any() and ((~el).any() or materials == "all")        # a closed box: every ray hits


def test_rgba_is_the_thresholds_applied_to_the_colours():
    cam, sp, col, cnt = rendered_frame(CPU, "cornell_glass", 33, 25)
    with g.Renderer(sp, 33, 25, cam, device=CPU) as r:
        r.write_radiance(col, cnt)
        for prm in (DEFAULTS, dict(DEFAULTS, materials="all", levels=2)):
            out, px = r.denoise(pixels=True, **prm)
            same(out, r.denoise(**prm), "with and without pixels")
            assert px.dtype == np.uint8 and np.array_equal(px, to_rgba(out))
        assert np.array_equal(r.read_pixels(), to_rgba(col))             # the context's own pixels: untouched
    assert len(np.unique(px[..., :3])) > 50 and not px[..., 3].any()


def test_errors():
    assert_errors(CPU)


def test_passes_after_denoise_equal_passes_without_it():
    assert_non_interference(CPU, "cornell_glass", 33, 25)


def test_denoising_four_passes_reduces_the_error():
    """Cornell 65x49 on the CPU backend with the reference's pass schedule: RMSE over all channels
    of the values clipped to [0, 1] against the 260-pass frame; with the default parameters the
    denoised 4-pass frame must be at <= 0.8 x the noisy one's (the prototype measured 0.671)."""
    W, H = 65, 49
    cam, sp = scene("cornell", W, H)
    sched = g.PassScheduler()
    with g.Renderer(sp, W, H, cam, device=CPU) as r:
        r.light_pass(0)
        sched.light()
        r.path_passes(*sched.next(4))
        noisy, _ = r.read_radiance()
        den = r.denoise()
        for _ in range(4):
            r.path_passes(*sched.next(64))
        ref, cnt = r.read_radiance()
    assert (cnt == 260).all()

    def rmse(a):
        d = np.clip(a.astype(np.float64), 0, 1) - np.clip(ref.astype(np.float64), 0, 1)
        return float(np.sqrt((d * d).mean()))

    e_noisy, e_den = rmse(noisy), rmse(den)
    print(f"RMSE vs 260 passes: noisy {e_noisy:.4f}, denoised {e_den:.4f}, ratio {e_den / e_noisy:.3f}")
    assert e_den <= 0.8 * e_noisy, (e_noisy, e_den)


def test_command_line_writes_the_denoised_frame(tmp_path):
    """smallpt 20 19 cornell.scn --spp 4 --device -1 --denoise --out x.ppm == save_ppm of
    Renderer.denoise(pixels=True) for the same schedule; the options reach the filter."""
    exe = os.path.join(REPO, "gpu_bidirectional_raytracer_amd", "smallpt")
    scn = os.path.join(SCENES, "cornell.scn")
    cam, sp, col, cnt = rendered_frame(CPU, "cornell", 21, 20)           # sizes get +1
    with g.Renderer(sp, 21, 20, cam, device=CPU) as r:
        r.write_radiance(col, cnt)
        for extra, prm in (([], {}), (["--denoise-levels", "2", "--denoise-sigma", "0.25", "--denoise-all"],
                                      dict(levels=2, sigma_color=0.25, materials="all"))):
            out = str(tmp_path / "x.ppm")
            subprocess.run([exe, "20", "19", scn, "--spp", "4", "--device", "-1", "--dat", g.DEFAULT_DAT, "--denoise",
                            "--out", out] + extra, check=True, cwd=REPO, capture_output=True, timeout=120)
            want = str(tmp_path / "want.ppm")
            g.save_ppm(want, r.denoise(pixels=True, **prm)[1])
            assert open(out, "rb").read() == open(want, "rb").read(), extra
        g.save_ppm(want, r.read_pixels())
        assert open(out, "rb").read() != open(want, "rb").read()         # not the raw frame
    r = subprocess.run([exe, "20", "19", scn, "--spp", "1", "--gpus", "2", "--denoise", "--out", out], cwd=REPO,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "--denoise needs one device" in r.stderr


def test_save_denoised_ppm_name_and_bytes(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    app = g.SmallPT(20, 19, os.path.join(SCENES, "cornell.scn"), device=CPU)
    app.IdleFunc()
    app.IdleFunc(3)
    raw = app.SavePPM()
    path = app.SaveDenoisedPPM()
    assert path == raw[:-4] + "_denoised.ppm" and os.path.exists(path)
    want = str(tmp_path / "want.ppm")
    g.save_ppm(want, app.renderer.denoise(pixels=True)[1])
    assert open(path, "rb").read() == open(want, "rb").read()
    p2 = app.SaveDenoisedPPM(str(tmp_path / "two.ppm"), binary=True, levels=2, materials="all")
    g.save_ppm(want, app.renderer.denoise(pixels=True, levels=2, materials="all")[1], binary=True)
    assert open(p2, "rb").read() == open(want, "rb").read()
    app.FreeBuffers()
