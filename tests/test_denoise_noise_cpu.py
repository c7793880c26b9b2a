"""The noise-guided denoiser (include/bdpt.h bdpt_denoise_noise) on the CPU backend
(device = BDPT_DEVICE_CPU, csrc/bdpt_cpu.cpp); runs without a GPU.

The definition is stated once more in numpy float32 (tests/denoise_noise_common.py np_denoise_noise)
and the backend must reproduce it bit for bit -- colours, pixels and the carried variance -- on
rendered frames with a mark between their passes and on synthetic frames whose counters and marks
sit on both sides of the validity rule.  Besides: the consequence that a frame without an estimate
gets bdpt_denoise's bits, the pass-through of a frame the mark calls noise-free, non-interference,
the error codes, RenderUntil(denoise=True), and what the filter is for -- its error against a
converged frame, next to the plain denoiser's and the raw frame's."""
import os
import subprocess
import sys

import numpy as np
import pytest

import gpu_bidirectional_raytracer_amd as g
from aov_common import same
from conftest import REPO, SCENES
from denoise_common import FRAMES
from denoise_noise_common import (CPU, F, SWEEP, SYNTHETIC, assert_equals_plain_denoise, assert_errors,
                                  assert_matches_numpy, assert_non_interference, assert_render_until,
                                  assert_zero_variance_passes_through, big_case, case, guides, raw_variance,
                                  rendered_marked, run)


@pytest.fixture(autouse=True)
def threads(monkeypatch):
    monkeypatch.setenv("BDPT_CPU_THREADS", "4")


@pytest.mark.parametrize("name,W,H", FRAMES, ids=lambda v: str(v))
def test_rendered_frames_equal_the_numpy_definition(name, W, H):
    cam, sp, col, cnt, mark = rendered_marked(CPU, name, W, H)
    with g.Renderer(sp, W, H, cam, device=CPU) as r:
        r.write_radiance(col, cnt)
        r.noise_write_mark(*mark)
        aov = r.render_aov()
        assert (raw_variance(col, cnt, *mark) >= 0).any()
        assert_matches_numpy(r, col, cnt, mark, aov["id"], aov["normal"], sp["refl"], f"{name} {W}x{H}")
        same(r.read_radiance()[0], col, "the accumulation is only read")
        same(r.noise_read_mark()[1], mark[1], "the mark is only read")
        assert r.last_denoise_noise_ms() >= 0.0


@pytest.mark.parametrize("name,W,H", SYNTHETIC, ids=lambda v: str(v))
def test_synthetic_frames_equal_the_numpy_definition(name, W, H):
    """Colours and marks with 0, -0, 1e-30 and 1e18, counts 0 .. 30000, marks on both sides of the
    validity boundary: pixels with and without an estimate sit next to each other."""
    col, cnt, mc, mn = case(W, H)
    cam, sp, ids, nrm = guides(name, W, H)
    v0 = raw_variance(col, cnt, mc, mn)
    assert (v0 >= 0).any() and (v0 < 0).any()
    with g.Renderer(sp, W, H, cam, device=CPU) as r:
        r.write_radiance(col, cnt)
        r.noise_write_mark(mc, mn)
        assert_matches_numpy(r, col, cnt, (mc, mn), ids, nrm, sp["refl"], f"synthetic {W}x{H}")
        again = run(r, **SWEEP[7])
        for a, b in zip(again, run(r, **SWEEP[7])):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), "a second call"


def test_counts_near_two_to_the_32():
    col, cnt, mc, mn = big_case()
    H, W = cnt.shape
    cam, sp, ids, nrm = guides("cornell_glass", W, H)
    v0 = raw_variance(col, cnt, mc, mn)
    big = cnt >= 2 ** 31
    assert ((v0 >= 0) & big).any() and ((v0 < 0) & big).any()
    with g.Renderer(sp, W, H, cam, device=CPU) as r:
        r.write_radiance(col, cnt)
        r.noise_write_mark(mc, mn)
        assert_matches_numpy(r, col, cnt, (mc, mn), ids, nrm, sp["refl"], "counts near 2^32", sweep=SWEEP[6:12])


def test_without_an_estimate_it_is_the_plain_denoiser():
    assert_equals_plain_denoise(CPU)


def test_zero_variance_passes_through():
    assert_zero_variance_passes_through(CPU)


def test_passes_after_the_call_equal_passes_without_it():
    assert_non_interference(CPU, "cornell_glass", 40, 33)


def test_error_codes():
    assert_errors(CPU)


def test_render_until_with_denoise():
    assert_render_until(CPU)


def test_save_denoised_ppm_with_noise(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    app = g.SmallPT(32, 24, os.path.join(SCENES, "cornell.scn"), device=CPU)
    try:
        app.IdleFunc(4)
        app.renderer.noise_mark()
        app.IdleFunc(4)
        name = app.SaveDenoisedPPM(noise=True, binary=True)
        assert name == app.SavePPM(binary=True)[:-len(".ppm")] + "_denoised_noise.ppm"
        _, px = app.renderer.denoise_noise(pixels=True, noise_sigma=2.0)
        g.save_ppm("by_hand.ppm", px, True)
        app.SaveDenoisedPPM("named.ppm", binary=True, noise=True, noise_sigma=2.0)
        assert open("named.ppm", "rb").read() == open("by_hand.ppm", "rb").read()
        assert open(name, "rb").read() != open("named.ppm", "rb").read()
    finally:
        app.FreeBuffers()


def test_smallpt_denoise_noise(tmp_path):
    """smallpt --until E --denoise-noise [S] writes the frame RenderUntil(denoise=True) filters; after
    --spp alone there is no mark and the file is --denoise's; several devices are refused."""
    exe = os.path.join(REPO, "gpu_bidirectional_raytracer_amd", "smallpt")
    scn = os.path.join(SCENES, "cornell.scn")
    base = [exe, "64", "48", scn, "--device", "-1", "--p6"]
    until = ["--until", "0.05", "--max-spp", "32", "--batch", "8"]

    def host(*args):
        r = subprocess.run(base + list(args), cwd=REPO, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        return r

    for sigma, extra in ((1.0, []), (2.0, ["2"])):
        out, want = str(tmp_path / f"c{sigma}.ppm"), str(tmp_path / f"py{sigma}.ppm")
        host(*until, "--denoise-noise", *extra, "--out", out)
        app = g.SmallPT(64, 48, scn, device=CPU)
        try:
            app.RenderUntil(threshold=0.05, max_passes=32, batch=8, denoise=True)
            g.save_ppm(want, app.renderer.denoise_noise(noise_sigma=sigma, pixels=True)[1], True)
        finally:
            app.FreeBuffers()
        assert open(out, "rb").read() == open(want, "rb").read(), sigma
    a, b, c = (str(tmp_path / n) for n in ("spp_noise.ppm", "spp_plain.ppm", "until_plain.ppm"))
    host("--spp", "8", "--denoise-noise", "--out", a)
    host("--spp", "8", "--denoise", "--out", b)
    host(*until, "--denoise", "--out", c)
    assert open(a, "rb").read() == open(b, "rb").read()
    assert open(c, "rb").read() != open(str(tmp_path / "c1.0.ppm"), "rb").read()
    r = subprocess.run(base + until + ["--denoise-noise", "--gpus", "2"], cwd=REPO, capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 1 and "--denoise-noise" in r.stderr


def test_noise_command_line_with_denoise(tmp_path):
    prefix = str(tmp_path / "n")
    scn = os.path.join(SCENES, "cornell.scn")
    cmd = [sys.executable, "-m", "gpu_bidirectional_raytracer_amd.noise", "64", "48", scn, "--until", "0.05",
           "--max-spp", "32", "--batch", "8", "--device", "-1", "--out", prefix, "--denoise", "--noise-sigma", "2"]
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    app = g.SmallPT(64, 48, scn, device=CPU)
    try:
        est = app.RenderUntil(0.05, max_passes=32, batch=8, pixels=True, denoise=True, noise_sigma=2.0)
    finally:
        app.FreeBuffers()
    z = np.load(prefix + ".npz")
    same(z["denoised"], est["denoised"], "the archive's filtered frame")
    same(z["variance"], est["denoised_variance"], "the archive's variance plane")
    same(z["error"], est["error"], "the archive's estimate")
    assert (z["variance"] >= 0).any()


# ---- what the filter is for ----------------------------------------------------------------------

def rmse(a, truth):
    d = np.clip(a, 0, 1).astype(np.float64) - np.clip(truth, 0, 1)
    return float(np.sqrt(np.mean(d * d)))


@pytest.fixture(scope="module")
def cornell_frames():
    """cornell at SmallPT(64, 48): for N = 8, 32, 128, 512 the raw frame, denoise() and denoise_noise()
    of it with the mark taken at N / 2, all with the defaults, and the 8192-pass frame as the truth.
    One render, snapshots on the way."""
    os.environ["BDPT_CPU_THREADS"] = "4"
    app = g.SmallPT(64, 48, os.path.join(SCENES, "cornell.scn"), device=CPU)
    out = {}
    try:
        for N in (8, 32, 128, 512):
            app.IdleFunc(N // 2 - app.current_sample)
            app.renderer.noise_mark()
            app.IdleFunc(N - app.current_sample)
            assert app.current_sample == N
            out[N] = (app.colors()[0], app.renderer.denoise(), app.renderer.denoise_noise())
        app.IdleFunc(8192 - app.current_sample)
        out["truth"] = app.colors()[0]
    finally:
        app.FreeBuffers()
    return out


def test_quality_against_a_converged_frame(cornell_frames):
    """RMSE of values clipped to [0, 1] against the 8192-pass frame.  The guided filter beats denoise()
    at 8, 32, 128 and 512 passes and is no worse than 1.1 x the raw frame at 512 (the margin: the
    truth's own noise, about 0.003, is a quarter of the raw error there).  Figures of this definition
    (raw, denoise, guided): 8: 0.0677 0.0485 0.0409; 32: 0.0382 0.0386 0.0269; 128: 0.0216 0.0351
    0.0181; 512: 0.0113 0.0337 0.0108."""
    truth = cornell_frames["truth"]
    for N in (8, 32, 128, 512):
        raw, plain, guided = (rmse(a, truth) for a in cornell_frames[N])
        print(f"cornell {N:4d} passes: raw {raw:.4f}  denoise {plain:.4f}  guided {guided:.4f}  "
              f"guided/denoise {guided / plain:.2f}  guided/raw {guided / raw:.2f}")
        assert guided < plain, N
        if N == 512:
            assert guided <= 1.1 * raw
