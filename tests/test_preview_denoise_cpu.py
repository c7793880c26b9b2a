"""The denoised preview (include/bdpt.h bdpt_preview_denoise) on the CPU backend
(device = BDPT_DEVICE_CPU, csrc/bdpt_cpu.cpp); runs without a GPU.

The definition is stated once more in numpy float32 (tests/preview_common.py np_preview_denoise, on
top of np_reproject) and the backend must reproduce it bit for bit.  Besides: the ties to the calls
that exist (levels = 0 is reproject(); a uniform 8-pass frame without history and count_ref = 8 is
denoise()), the synthetic case with holes and absurd weights, the error codes, side effects, the
interactive mirror and the command line, and two statistical tests: that the count weighting beats
the same filter told a uniform count, and that after a camera key the denoised preview is closer to
the converged frame than reproject() or denoise() alone."""
import os
import subprocess

import numpy as np
import pytest

import gpu_bidirectional_raytracer_amd as g
from aov_common import same, scene
from conftest import REPO, SCENES
from preview_common import (CPU, F, FRAMES, HI, INF, LO, MOVES, SYNTHETIC, SYNTHETIC_PARAMS, assert_errors,
                            assert_identity_with_denoise, assert_levels0_is_reproject, assert_non_interference,
                            case_of, clampc, eligible, first_hit, hist_dict, history_of, moved, np_preview_denoise,
                            np_preview_levels, np_reproject, params_of, results, synthetic_inputs, synthetic_results,
                            to_rgba)

IDS = lambda k: "+".join(k).replace(" ", "space")


@pytest.fixture(autouse=True)
def threads(monkeypatch):
    monkeypatch.setenv("BDPT_CPU_THREADS", "4")


# ---- A. the statement -------------------------------------------------------------------------
@pytest.mark.parametrize("keys", MOVES, ids=IDS)
@pytest.mark.parametrize("name,W,H,traversal", FRAMES)
def test_cpu_backend_equals_the_numpy_definition(name, W, H, traversal, keys):
    cam0, sp, hc, hm, aov0 = history_of(name, W, H)
    cam1, col, cnt, aov1 = case_of(name, W, H, keys)
    hist = hist_dict(cam0, hc, hm, aov0)
    got = results(CPU, name, W, H, traversal, keys)
    changed = 0
    for prm, (c, w, px) in zip(params_of(W, H), got):
        what = f"{name} {W}x{H} {keys} {prm}"
        o, a, tot = np_preview_denoise(col, cnt, aov1, sp["refl"], hist, **prm)
        same(c, o, what + ": colours")
        same(w, a, what + ": count")
        assert np.array_equal(px, to_rgba(o)), what
        assert not np.isnan(c).any() and not np.isnan(w).any(), what
        if prm["levels"]:
            changed += int((o != np_reproject(col, cnt, aov1, sp["refl"], hist, prm["max_history"], 0.01,
                                              prm["materials"])[0]).any())
    assert changed, "no parameter set filtered anything"


def test_numpy_statement_of_identity_b_first():
    """Uniform counts stay exactly uniform and scale out of the statement: with every count 8 and
    count_ref = 8 the levels are np_denoise's, in numpy before any backend is asked."""
    from denoise_common import np_denoise, rendered_frame
    cam, sp, col, cnt = rendered_frame(CPU, "cornell", 33, 25, npass=8)
    with g.Renderer(sp, 33, 25, cam, device=CPU) as r:
        aov = r.render_aov()
    for levels in (1, 3, 5):
        for npow in (0, 5):
            want = np_denoise(col, aov["id"], aov["normal"], sp["refl"], levels=levels, normal_power=npow)
            got, a = np_preview_levels(col, cnt.astype(F), aov["id"], aov["normal"], sp["refl"], levels, npow, 0.5, 8.0,
                                       "diffuse")
            same(got, want, f"numpy: levels {levels} normal_power {npow}")
            assert (a == 8).all()


def test_synthetic_history_with_holes_and_absurd_weights():
    """History colours with 0, -0, 1e-30 and 1e18, weights 0 .. 1e30 in blocks, from a reset
    accumulation (n == 0: holes next to filled pixels) and after one pass."""
    name, W, H, keys = SYNTHETIC
    cam0, cam1, sp, hc, hm, col1, cnt1 = synthetic_inputs()
    aov0, aov1 = first_hit(sp, W, H, cam0), first_hit(sp, W, H, cam1)
    hist = hist_dict(cam0, hc, hm, aov0)
    zero = np.zeros((H, W, 3), F), np.zeros((H, W), np.uint32)
    res = synthetic_results(CPU)
    seen = dict(hole_filled=0, hole_kept=0, low=0, high=0, finite=0)
    for (col, cnt), per_state in zip((zero, (col1, cnt1)), res):
        for prm, (c, w, px) in zip(SYNTHETIC_PARAMS, per_state):
            what = f"synthetic n={'1' if cnt.any() else '0'} {prm}"
            o, a, tot = np_preview_denoise(col, cnt, aov1, sp["refl"], hist, **prm)
            same(c, o, what + ": colours")
            same(w, a, what + ": count")
            assert np.array_equal(px, to_rgba(o)), what
            # the reprojection's own blend overflows where n >= 1 meets m = 1e30 and a colour of 1e18
            # (bdpt_reproject: non-finite radiance is not special); everywhere else the input to the
            # levels is finite and no NaN may appear
            if np.isfinite(np_reproject(col, cnt, aov1, sp["refl"], hist, prm["max_history"], 0.01,
                                        prm["materials"])[0]).all():
                assert not np.isnan(c).any() and not np.isnan(w).any(), what
                seen["finite"] += 1
            assert ((w == 0) | ((w >= LO) & (w <= HI))).all(), what
            e = eligible(aov1["id"], sp["refl"], prm["materials"])
            hole = e & (tot == 0)
            seen["hole_filled"] += int((hole & (w > 0)).sum())                # the a_p == 0 branch
            kept = hole & (w == 0)
            seen["hole_kept"] += int(kept.sum())
            assert (c[kept] == col[kept]).all(), what                          # no tap used: cur[p], count 0
            seen["low"] += int(((tot > 0) & (tot < LO)).sum())                  # both clamps at entry
            seen["high"] += int((tot > HI).sum())
    assert seen["hole_filled"] and seen["hole_kept"] and seen["low"] and seen["high"], seen
    assert seen["finite"] >= 5, seen                               # every reset-accumulation case among them


def test_a_centre_without_a_count_is_not_its_own_tap():
    """One hole among pixels of unequal colour: the hole's output is the count-weighted mean of its
    neighbours alone (wc = 1), and its own stale colour plays no part."""
    W, H = 7, 5
    ids = np.zeros((H, W), np.int32)
    nrm = np.zeros((H, W, 3), F)
    nrm[..., 2] = 1
    rng = np.random.default_rng(3)
    col = rng.random((H, W, 3), dtype=F)
    tot = np.full((H, W), 4, F)
    tot[2, 3] = 0
    refl = np.array([g.DIFF])
    out1, cnt1 = np_preview_levels(col, tot, ids, nrm, refl, 1, 5, 0.5, 8.0, "all")
    col2 = col.copy()
    col2[2, 3] = 1e6                                               # a different stale colour in the hole
    out2, _ = np_preview_levels(col2, tot, ids, nrm, refl, 1, 5, 0.5, 8.0, "all")
    same(out1[2, 3], out2[2, 3], "the hole's output does not depend on its own colour")
    assert cnt1[2, 3] == 4                                           # and it carries its neighbours' count


# ---- B. ties to the code that exists ----------------------------------------------------------
@pytest.mark.parametrize("keys", MOVES[:2], ids=IDS)
def test_levels_0_is_reproject(keys):
    assert_levels0_is_reproject(CPU, "cornell", 65, 49, keys)
    assert_levels0_is_reproject(CPU, "caustic", 40, 33, keys)


@pytest.mark.parametrize("name,W,H", [("cornell", 33, 25), ("cornell_glass", 65, 49)])
def test_uniform_eight_passes_without_history_is_denoise(name, W, H):
    assert_identity_with_denoise(CPU, name, W, H)


# ---- C. the count weighting earns its place ---------------------------------------------------
def test_count_weighting_beats_a_uniform_count():
    """One wall, camera unchanged, n == 0; history = a constant + seeded noise of standard deviation
    sigma / sqrt(hm), hm in 4 x 4 blocks of 1 and 64.  RMSE against the constant over interior
    pixels: the call told the true counts < the same call on the same colours told the mean count
    everywhere, and < the unfiltered input."""
    W, H = 65, 49
    cam, sp = scene("cornell", W, H)
    with g.Renderer(sp, W, H, cam, device=CPU) as r:
        ids = r.render_aov()["id"]
    wall = np.bincount(ids[ids >= 0]).argmax()
    sp1 = sp[wall:wall + 1].copy()
    rng = np.random.default_rng(11)
    y, x = np.mgrid[0:H, 0:W]
    hm = np.where(((x // 4) + (y // 4)) % 2 == 0, F(1), F(64)).astype(F)
    const, sigma = np.array([0.5, 0.4, 0.3], F), 0.2
    hc = (const + rng.standard_normal((H, W, 3)).astype(F) * (F(sigma) / np.sqrt(hm))[..., None]).astype(F)
    mean = np.full((H, W), hm.mean(), F)
    with g.Renderer(sp1, W, H, cam, device=CPU) as r:
        assert (r.render_aov()["id"] == 0).all()                   # one wall fills the frame
        r.history_write(cam, hc, hm)
        raw, tot = r.reproject(materials="all", weight=True)
        counted = r.preview_denoise(materials="all")
        r.history_write(cam, hc, mean)
        uniform = r.preview_denoise(materials="all")
    assert (tot[8:-8, 8:-8] > 0).all()

    def rmse(a):
        d = a[8:-8, 8:-8].astype(np.float64) - const
        return float(np.sqrt((d * d).mean()))

    e_raw, e_cnt, e_uni = rmse(raw), rmse(counted), rmse(uniform)
    print(f"RMSE vs the constant: input {e_raw:.5f}, true counts {e_cnt:.5f}, mean count {e_uni:.5f}")
    assert e_cnt < e_uni, (e_cnt, e_uni)
    assert e_cnt < e_raw, (e_cnt, e_raw)


# ---- D. quality -------------------------------------------------------------------------------
# ratio of preview_denoise's RMSE to reproject()'s measured when the call was written: 0.955 for
# `left` (0.0592 / 0.0620), 0.933 for `a` (0.0742 / 0.0795); the limit is halfway between that and 1
RATIO_LIMIT = {("left",): (0.955 + 1) / 2, ("a",): (0.933 + 1) / 2}


@pytest.mark.parametrize("keys", [("left",), ("a",)], ids=IDS)
def test_denoised_preview_after_a_camera_key_is_closer_to_the_converged_frame(keys):
    """Cornell 65x49: 16 passes, capture, the key, ReInit's reset and one pass; 260 passes of the new
    view as the truth.  RMSE over all channels of the values clipped to [0, 1]: preview_denoise is
    below reproject() alone (recorded: 0.0620 for `left`, 0.0795 for `a`) and below denoise() of the
    one-pass frame alone."""
    W, H = 65, 49
    cam0, sp = scene("cornell", W, H)
    cam1 = moved(cam0, keys, W, H)
    sched = g.PassScheduler()
    with g.Renderer(sp, W, H, cam0, device=CPU) as r:
        r.light_pass(0)
        sched.light()
        r.path_passes(*sched.next(16))
        r.history_capture()
        r.reset_accum()
        r.set_camera(cam1)
        r.path_passes(*sched.next(1))
        preview = r.reproject()
        denoised = r.denoise()
        both = r.preview_denoise()
        r.path_passes(*sched.next(3))
        for _ in range(4):
            r.path_passes(*sched.next(64))
        ref, cnt = r.read_radiance()
    assert (cnt == 260).all()

    def rmse(a):
        d = np.clip(a.astype(np.float64), 0, 1) - np.clip(ref.astype(np.float64), 0, 1)
        return float(np.sqrt((d * d).mean()))

    e_prev, e_dn, e_both = rmse(preview), rmse(denoised), rmse(both)
    print(f"{keys}: RMSE vs 260 passes: reproject {e_prev:.4f}, denoise {e_dn:.4f}, preview_denoise {e_both:.4f}, "
          f"ratio to reproject {e_both / e_prev:.3f}")
    assert e_both < e_prev and e_both < e_dn, (e_prev, e_dn, e_both)
    assert e_both / e_prev <= RATIO_LIMIT[keys], (e_both / e_prev, RATIO_LIMIT[keys])


# ---- E. non-interference ----------------------------------------------------------------------
def test_passes_after_the_call_equal_passes_without_it():
    assert_non_interference(CPU, "cornell_glass", 33, 25)


# ---- F. errors --------------------------------------------------------------------------------
def test_errors():
    assert_errors(CPU)


# ---- G. the mirror and the command line -------------------------------------------------------
def _drive(app):
    app.IdleFunc()
    app.IdleFunc(3)
    app.KeyFunc("a")
    app.IdleFunc(4)
    app.SpecialFunc("left")
    app.IdleFunc(4)


def test_mirror_preview_and_file_names(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    app = g.SmallPT(20, 19, os.path.join(SCENES, "cornell.scn"), device=CPU, reuse_history=True)
    _drive(app)
    same(app.preview(), app.renderer.reproject(), "preview() is unchanged")
    same(app.preview(denoise=True), app.renderer.preview_denoise(), "preview(denoise=True)")
    same(app.preview(denoise=True, count_ref=2.0, levels=2), app.renderer.preview_denoise(count_ref=2.0, levels=2),
         "preview(denoise=True, ...)")
    raw = app.SavePPM()
    assert app.SavePreviewPPM() == raw[:-4] + "_preview.ppm"
    path = app.SavePreviewPPM(denoise=True)
    assert path == raw[:-4] + "_preview_denoised.ppm" and os.path.exists(path)
    want = str(tmp_path / "want.ppm")
    g.save_ppm(want, app.renderer.preview_denoise(pixels=True)[1])
    assert open(path, "rb").read() == open(want, "rb").read()
    assert open(path, "rb").read() != open(raw[:-4] + "_preview.ppm", "rb").read()
    app.FreeBuffers()


def test_command_line_writes_the_denoised_preview(tmp_path):
    """smallpt 20 19 cornell.scn --spp 4 --keys aL --device -1 --reproject --denoise --out x.ppm ==
    SavePreviewPPM(denoise=True) of the mirror driven through the same keys and passes; the
    --denoise-* options reach the call; each option alone behaves as before."""
    exe = os.path.join(REPO, "gpu_bidirectional_raytracer_amd", "smallpt")
    scn = os.path.join(SCENES, "cornell.scn")
    app = g.SmallPT(20, 19, scn, device=CPU, reuse_history=True)
    _drive(app)
    out, want = str(tmp_path / "x.ppm"), str(tmp_path / "want.ppm")
    base = [exe, "20", "19", scn, "--spp", "4", "--keys", "aL", "--device", "-1", "--dat", g.DEFAULT_DAT, "--out", out]
    run = lambda extra: subprocess.run(base + extra, check=True, cwd=REPO, capture_output=True, timeout=120)
    run(["--reproject", "--denoise"])
    app.SavePreviewPPM(want, denoise=True)
    both = open(out, "rb").read()
    assert both == open(want, "rb").read()
    run(["--reproject", "--denoise", "--denoise-count", "2", "--denoise-levels", "2"])
    app.SavePreviewPPM(want, denoise=True, count_ref=2.0, levels=2)
    assert open(out, "rb").read() == open(want, "rb").read() and open(out, "rb").read() != both
    run(["--reproject", "--denoise", "--denoise-all", "--denoise-sigma", "0.1"])
    app.SavePreviewPPM(want, denoise=True, materials="all", sigma_color=0.1)
    assert open(out, "rb").read() == open(want, "rb").read()
    run(["--reproject"])                                           # each option alone: as before
    app.SavePreviewPPM(want)
    assert open(out, "rb").read() == open(want, "rb").read() and open(out, "rb").read() != both
    run(["--denoise"])
    app.SaveDenoisedPPM(want)
    assert open(out, "rb").read() == open(want, "rb").read() and open(out, "rb").read() != both
    app.FreeBuffers()
    r = subprocess.run(base + ["--reproject", "--denoise", "--gpus", "2"], cwd=REPO, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 1 and "--denoise needs one device" in r.stderr
    r = subprocess.run(base + ["--reproject", "--gpus", "2"], cwd=REPO, capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "--reproject needs one device" in r.stderr
