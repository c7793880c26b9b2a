"""The per-tile noise estimate (include/bdpt.h bdpt_noise_estimate and the mark's entry points) on the
CPU backend (device = BDPT_DEVICE_CPU, csrc/bdpt_cpu.cpp); runs without a GPU.

The definition is stated once more in numpy float32 (tests/noise_common.py np_noise) and the backend
must reproduce it bit for bit -- the per-pixel plane, the tile arrays, the summary and the mark after
re-marking -- on synthetic frames whose counters and marks sit on both sides of every rule.  Besides:
the error codes, the five calls that clear the mark, the mark's round trip, what the estimate means
on rendered frames (two conditions, not measurements), RenderUntil against the statement driven from
outside, and the two command lines."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import gpu_bidirectional_raytracer_amd as g
from aov_common import same, scene
from conftest import REPO, SCENES
from noise_common import (CAP, CPU, F, FRAMES, PARAMS, TH, TW, assert_errors, big_case, case, np_noise,
                          np_render_until, rendered_pair, run_arrays, run_case, same_estimate, same_summary, want_case)

SCN = os.path.join(SCENES, "cornell.scn")


@pytest.fixture(autouse=True)
def threads(monkeypatch):
    monkeypatch.setenv("BDPT_CPU_THREADS", "4")


@pytest.mark.parametrize("remark", [False, True], ids=["plain", "remark"])
@pytest.mark.parametrize("W,H", FRAMES, ids=lambda v: str(v))
def test_cpu_backend_equals_the_numpy_definition(W, H, remark):
    for prm in PARAMS:
        same_estimate(run_case(CPU, W, H, remark, **prm), want_case(W, H, remark, **prm), f"{W}x{H} {prm}")


def test_the_cases_cover_the_rules():
    """A tile without a valid pixel, a tile with all 256 valid, both sides of the fresh-sample
    boundary -- (mn, cnt) = (2, 3) valid, (3, 4) not -- pending pixels, pixels at the cap, and pixels
    that take and that do not take the mark."""
    none = full = False
    seen = set()
    for W, H in FRAMES:
        col, cnt, mc, mn = case(W, H)
        w = np_noise(col, cnt, mc, mn, remark=True)
        none |= bool((w["tile_valid"] == 0).any())
        full |= bool((w["tile_valid"] == TW * TH).any())
        valid = w["error"] >= 0
        assert ((w["error"] == F(-1)) == ~valid).all()
        for pair in ((2, 3), (3, 4)):
            at = (mn == pair[0]) & (cnt == pair[1])
            if at.any():
                seen.add((pair, bool(valid[at].all()), bool(valid[at].any())))
        took = w["mark"][1] != mn
        if W * H > 256:
            assert took.any() and (~took & (cnt > 0)).any() and (w["tile_pending"] > 0).any()
            assert ((cnt == CAP) & valid).any() and ((cnt == CAP) & ~valid & ~took).any()
    assert none and full
    assert ((2, 3), True, True) in seen and ((3, 4), False, False) in seen


@pytest.mark.parametrize("remark", [False, True], ids=["plain", "remark"])
def test_counts_near_two_to_the_32(remark):
    col, cnt, mc, mn = big_case()
    want = np_noise(col, cnt, mc, mn, remark=remark)
    same_estimate(run_arrays(CPU, col, cnt, mc, mn, remark), want, "counts near 2^32")
    valid = want["error"] >= 0
    big = cnt >= 2 ** 31
    assert (valid & big).any() and (~valid & big).any() and want["pending_pixels"] > 0
    if remark:
        assert (want["mark"][1] != mn).any() and (want["mark"][1][big] == mn[big]).all()


def test_error_codes():
    assert_errors(CPU)


def test_mark_round_trip_and_first_mark():
    W, H = 33, 9
    col, cnt, mc, mn = case(W, H)
    cam, sp = scene("cornell", W, H)
    with g.Renderer(sp, W, H, cam, device=CPU) as r:
        r.write_radiance(col, cnt)
        r.noise_write_mark(mc, mn)
        got = r.noise_read_mark()
        same(got[0], mc, "round trip: colours")
        same(got[1], mn, "round trip: counts")
        r.noise_mark()
        got = r.noise_read_mark()
        same(got[0], col, "noise_mark: colours")
        same(got[1], cnt, "noise_mark: counts")
        r.noise_clear()
        same(r.noise_read_mark()[1], np.zeros_like(cnt), "noise_clear: counts")
    with g.Renderer(sp, W, H, cam, device=CPU) as r:          # an unmarked context: remark takes the mark
        r.write_radiance(col, cnt)
        est = r.noise_estimate(remark=True)
        assert est["valid_pixels"] == 0 and est["valid_tiles"] == 0 and est["mean"] == 0.0 and est["max_tile"] == 0.0
        assert est["pending_pixels"] == int(((cnt > 0) & (cnt < CAP)).sum())
        got = r.noise_read_mark()
        grow = (cnt > 0) & (cnt < CAP)
        same(got[1], np.where(grow, cnt, 0).astype(np.uint32), "first mark: counts")
        same(got[0][grow], col[grow], "first mark: colours")
        want = np_noise(col, cnt, got[0], got[1], remark=False)
        same_estimate(r.noise_estimate(pixels=True), want, "after the first mark")


@pytest.mark.parametrize("call", ["reset_accum", "set_scene", "set_camera", "write_radiance", "load_checkpoint"])
def test_calls_that_rewrite_the_accumulation_clear_the_mark(call, tmp_path):
    W, H = 33, 9
    col, cnt, mc, mn = case(W, H)
    cam, sp = scene("cornell", W, H)
    ck = str(tmp_path / "frame.ckpt")
    with g.Renderer(sp, W, H, cam, device=CPU) as r:
        r.light_pass(0)
        r.write_radiance(col, cnt)
        if call == "load_checkpoint":
            r.save_checkpoint(ck, b"")
        r.noise_write_mark(mc, mn)
        assert r.noise_estimate()["valid_pixels"] > 0
        if call == "reset_accum":
            r.reset_accum()
        elif call == "set_scene":
            r.set_scene(sp)
        elif call == "set_camera":
            r.set_camera(cam)
        elif call == "write_radiance":
            r.write_radiance(col, cnt)
        else:
            r.load_checkpoint(ck, 0)
        if call == "reset_accum":
            r.write_radiance(col, cnt)                        # (clears again; the counters are back)
        est = r.noise_estimate()
        assert est["valid_pixels"] == 0 and est["tiles_over"] == 0
        same(r.noise_read_mark()[1], np.zeros_like(mn), f"{call}: the mark's counts")


def _true_mean(frame, ref, dark=0.01):
    """The per-pixel formula with the converged frame in the mark's place and no count scaling."""
    b, r = frame.astype(np.float64), ref.astype(np.float64)
    e1 = np.abs(b - r).sum(axis=2)
    return float((e1 / np.sqrt(np.maximum(b.sum(axis=2), dark))).mean())


@pytest.fixture(scope="module")
def meaning():
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("BDPT_CPU_THREADS", "4")
        est16, col16 = rendered_pair(CPU, 8, 8)
        est128, col128 = rendered_pair(CPU, 64, 64)
        app = g.SmallPT(64, 48, SCN, device=CPU)
        try:
            app.IdleFunc(1024)
            ref = app.colors()[0]
        finally:
            app.FreeBuffers()
    return est16, col16, est128, col128, ref


def test_the_estimate_falls_with_the_pass_count(meaning):
    """Condition 1: the frame mean at 128 passes (mark at 64) is below the one at 16 (mark at 8)."""
    est16, _, est128, _, _ = meaning
    assert est16["valid_pixels"] == est128["valid_pixels"] == 65 * 49
    print("frame mean at 16 passes", est16["mean"], "at 128 passes", est128["mean"])
    assert est128["mean"] < est16["mean"]


def test_the_estimate_is_within_a_factor_of_two_of_the_true_error(meaning):
    """Condition 2: each frame mean against the mean error measured with a 1024-pass frame."""
    est16, col16, est128, col128, ref = meaning
    for est, col, n in ((est16, col16, 16), (est128, col128, 128)):
        truth = _true_mean(col, ref)
        print(f"{n} passes: estimate {est['mean']:.5f}, true {truth:.5f}, ratio {est['mean'] / truth:.3f}")
        assert 0.5 <= est["mean"] / truth <= 2.0


@pytest.fixture(scope="module")
def until():
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("BDPT_CPU_THREADS", "4")
        app = g.SmallPT(64, 48, SCN, device=CPU)
        try:
            got = app.RenderUntil(0.05, max_passes=1024, batch=8)
            frame = app.colors()
        finally:
            app.FreeBuffers()
    return got, frame


def test_render_until_equals_the_statement_driven_from_outside(until):
    got, frame = until
    want, col, cnt = np_render_until(CPU, 0.05, 1024, 8)
    print("RenderUntil stopped at", got["passes"], "passes; worst tile", got["max_tile"], "mean", got["mean"])
    assert got["passes"] == want["passes"] and got["converged"] == want["converged"]
    same_summary(got, want, "RenderUntil's summary")
    same(got["tile_error"], want["tile_error"], "RenderUntil: tile_error")
    same(got["tile_valid"], want["tile_valid"], "RenderUntil: tile_valid")
    same(frame[0], col, "non-interference: colours")
    same(frame[1], cnt, "non-interference: counters")
    assert got["converged"] and got["passes"] < 1024 and got["passes"] % 8 == 0
    assert got["max_tile"] <= 0.05 and got["pending_pixels"] == 0


def test_render_until_gives_up_at_max_passes():
    app = g.SmallPT(64, 48, SCN, device=CPU)
    try:
        got = app.RenderUntil(0.05, max_passes=16, batch=8)
        assert got["converged"] is False and got["passes"] == 16 == app.current_sample
        assert got["valid_pixels"] == 65 * 49                 # marked at 8, estimated at 16
    finally:
        app.FreeBuffers()


def test_smallpt_until(tmp_path):
    """smallpt 64 48 cornell.scn --device -1 --until 0.05 --max-spp 64 --batch 8: the report line
    carries RenderUntil's stop point, worst tile and mean, and --out the same frame; after a camera
    key the mark starts afresh; several devices are refused."""
    exe = os.path.join(REPO, "gpu_bidirectional_raytracer_amd", "smallpt")
    out, want = str(tmp_path / "c.ppm"), str(tmp_path / "py.ppm")
    base = [exe, "64", "48", SCN, "--device", "-1", "--until", "0.05", "--max-spp", "64", "--batch", "8"]
    r = subprocess.run(base + ["--out", out], cwd=REPO, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    app = g.SmallPT(64, 48, SCN, device=CPU)
    try:
        est = app.RenderUntil(0.05, max_passes=64, batch=8)
        app.SavePPM(want)
        lines = re.findall(r"^Until 0\.05: (\d+) passes \((\d+) in this render\), (converged|not converged), "
                           r"worst tile (\S+), mean (\S+)$", r.stderr, re.M)
        assert len(lines) == 1
        n, fresh, word, worst, mean = lines[0]
        assert int(n) == int(fresh) == est["passes"] == 64 and word == "not converged" and not est["converged"]
        assert F(float(worst)) == F(est["max_tile"]) and float(mean) == est["mean"]
        assert open(out).read() == open(want).read()
    finally:
        app.FreeBuffers()
    app = g.SmallPT(64, 48, SCN, device=CPU)
    try:
        app.RenderUntil(0.05, max_passes=24, batch=8)
        app.KeyFunc("a")
        est2 = app.RenderUntil(0.05, max_passes=24, batch=8)
    finally:
        app.FreeBuffers()
    r = subprocess.run(base[:-4] + ["--max-spp", "24", "--batch", "8", "--keys", "a"], cwd=REPO, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = re.findall(r"^Until 0\.05: (\d+) passes \((\d+) in this render\), (\S+ ?\S*), worst tile (\S+), mean (\S+)$",
                       r.stderr, re.M)
    assert len(lines) == 2 and int(lines[1][0]) == est2["passes"] == 25 and int(lines[1][1]) == 24
    assert F(float(lines[1][3])) == F(est2["max_tile"]) and float(lines[1][4]) == est2["mean"]
    for many in (["--gpus", "2"], ["--devices", "0,1"]):
        r = subprocess.run(base + many, cwd=REPO, capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and "--until needs one device" in r.stderr


def test_noise_module_command_line(tmp_path):
    """python -m gpu_bidirectional_raytracer_amd.noise: the archive holds RenderUntil's last estimate,
    the heat map its per-pixel plane."""
    prefix = str(tmp_path / "n")
    cmd = [sys.executable, "-m", "gpu_bidirectional_raytracer_amd.noise", "64", "48", SCN, "--until", "0.05",
           "--max-spp", "32", "--batch", "8", "--device", "-1", "--out", prefix, "--ppm"]
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    app = g.SmallPT(64, 48, SCN, device=CPU)
    try:
        est = app.RenderUntil(0.05, max_passes=32, batch=8, pixels=True)
    finally:
        app.FreeBuffers()
    z = np.load(prefix + ".npz")
    assert sorted(z.files) == ["error", "summary", "tile_error", "tile_valid"]
    for k in ("error", "tile_error", "tile_valid"):
        same(z[k], est[k], f"npz: {k}")
    s = z["summary"]
    for k in ("valid_pixels", "pending_pixels", "tiles_x", "tiles_y", "valid_tiles", "tiles_over", "passes"):
        assert int(s[k]) == est[k], k
    assert float(s["mean"]) == est["mean"] and F(s["max_tile"]) == F(est["max_tile"])
    assert bool(s["converged"]) == est["converged"] and int(s["passes"]) == 32 and F(s["threshold"]) == F(0.05)
    assert f"65x49: 32 passes, not converged" in r.stderr
    from gpu_bidirectional_raytracer_amd.noise import error_rgba
    want = str(tmp_path / "want.ppm")
    g.save_ppm(want, error_rgba(est["error"], 0.05))
    assert open(prefix + "_error.ppm").read() == open(want).read()
    grey = error_rgba(est["error"], 0.05)
    assert grey.shape == (49, 65, 4) and grey[..., 0].max() > 0 and (grey[..., 0] == grey[..., 2]).all()
