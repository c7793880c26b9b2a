"""Temporal reprojection (include/bdpt.h bdpt_reproject and the history entry points) on the CPU
backend (device = BDPT_DEVICE_CPU, csrc/bdpt_cpu.cpp); runs without a GPU.

The definition is stated once more in numpy float32 (tests/reproject_common.py np_reproject) and the
backend must reproduce it bit for bit: histories and one-pass frames of four scenes over camera
moves and the parameter sweep, uneven and zero history weights, synthetic radiance, a two-step
chain of captures.  Besides: a geometric check of the fetch that does not use the statement's
projection, what the validation rejects, the 8-bit pixels, the error codes, side effects, the
interactive mirror, the command line, and the one statistical test -- that the preview after a
camera key is closer to the converged frame than the raw one-pass frame."""
import os
import subprocess

import numpy as np
import pytest

import gpu_bidirectional_raytracer_amd as g
from aov_common import same, scene
from conftest import REPO, SCENES
from reproject_common import (CPU, DEFAULTS, F, FRAMES, INF, KEYSETS, MOVES, SWEEP, assert_errors,
                              assert_non_interference, assert_sweep, case_of, eligible, first_hit, hist_dict,
                              history_of, moved, np_reproject, patterned_weight, rendered, synthetic_radiance, to_rgba)


@pytest.fixture(autouse=True)
def threads(monkeypatch):
    monkeypatch.setenv("BDPT_CPU_THREADS", "4")


@pytest.mark.parametrize("keys", KEYSETS, ids=lambda k: "+".join(k).replace(" ", "space"))
@pytest.mark.parametrize("name,W,H,traversal", FRAMES)
def test_cpu_backend_equals_the_numpy_definition(name, W, H, traversal, keys):
    want = assert_sweep(CPU, name, W, H, traversal, keys)
    cam1, col, cnt, aov1 = case_of(name, W, H, keys)
    took = [int((w != cnt.astype(F)).sum()) for _, w in want]
    assert max(took) > 0, "no pixel took history"
    if len(keys) == 7 and (W, H) != (7, 5):
        assert min(took) < cnt.size // 2                       # much of the frame is outside the old view
    if name in ("caustic", "complex"):
        assert (aov1["id"] < 0).any()


@pytest.mark.parametrize("keys", KEYSETS, ids=lambda k: "+".join(k).replace(" ", "space"))
def test_history_with_a_different_count_per_pixel(keys):
    W, H = 65, 49
    hm = patterned_weight(W, H)
    assert (hm == 0).any() and len(np.unique(hm)) == 5
    assert_sweep(CPU, "cornell", W, H, None, keys, hm=hm, params=[DEFAULTS, SWEEP[-1], dict(DEFAULTS, max_history=1.0)])


@pytest.mark.parametrize("materials", ["diffuse", "all"])
def test_synthetic_radiance_and_pixels_without_samples(materials):
    """History and frame of seeded values with 0, -0, 1e-30 and 1e18; counters 0..3 from pixel to
    pixel, so that n == 0 meets both m > 0 (out = h) and m == 0 (out = the stale colour)."""
    name, W, H = "cornell_glass", 40, 33
    cam0, sp = scene(name, W, H)
    hc, col = synthetic_radiance(W, H), synthetic_radiance(W, H, seed=7)
    hm = patterned_weight(W, H)
    y, x = np.mgrid[0:H, 0:W]
    cnt = ((x + 2 * y) % 4).astype(np.uint32)
    aov0 = first_hit(sp, W, H, cam0)
    for keys in MOVES[:2]:
        cam1 = moved(cam0, keys, W, H)
        aov1 = first_hit(sp, W, H, cam1)
        with g.Renderer(sp, W, H, cam1, device=CPU) as r:
            r.write_radiance(col, cnt)
            r.history_write(cam0, hc, hm)
            for mh, tol in ((INF, 0.0), (1.0, INF), (64.0, 0.01)):
                prm = dict(materials=materials, max_history=mh, plane_tol=tol)
                o, w, taps = np_reproject(col, cnt, aov1, sp["refl"], hist_dict(cam0, hc, hm, aov0), **prm)
                got, gw = r.reproject(weight=True, **prm)
                same(got, o, f"synthetic {keys} {prm}: out")
                same(gw, w, f"synthetic {keys} {prm}: weight")
                same(r.reproject(**prm), got, "a second call")
        m = w - cnt.astype(F)
        assert ((cnt == 0) & (m > 0)).any() and ((cnt == 0) & (m == 0)).any() and ((cnt > 0) & (m > 0)).any()
        same(got[(cnt == 0) & (m == 0)], col[(cnt == 0) & (m == 0)], "no samples and no history: the stale colour")


def test_two_captures_in_a_chain():
    """capture, move, one pass, capture, move, one pass, reproject == the statement applied twice."""
    name, W, H = "cornell", 65, 49
    cam0, sp, colA, hmA, aov0 = history_of(name, W, H)
    cam1, colB, cntB, aov1 = case_of(name, W, H, ("a",))
    cam2 = moved(cam1, ("left",), W, H)
    colC, cntC = rendered(CPU, sp, W, H, cam2, 1)
    aov2 = first_hit(sp, W, H, cam2)
    with g.Renderer(sp, W, H, cam0, device=CPU) as r:
        r.write_radiance(colA, hmA.astype(np.uint32))
        r.history_capture()
        assert r.history_info()[0] and bytes(r.history_info()[1]) == bytes(cam0)
        r.set_camera(cam1)
        r.write_radiance(colB, cntB)
        r.history_capture()
        assert bytes(r.history_info()[1]) == bytes(cam1)
        r.set_camera(cam2)
        r.write_radiance(colC, cntC)
        got, gw = r.reproject(weight=True)
    o1, w1, _ = np_reproject(colB, cntB, aov1, sp["refl"], hist_dict(cam0, colA, hmA, aov0))
    o2, w2, _ = np_reproject(colC, cntC, aov2, sp["refl"], hist_dict(cam1, o1, w1, aov1))
    same(got, o2, "chain: out")
    same(gw, w2, "chain: weight")
    assert (w2 > 5).any()                                      # 1 + (1 + 4): history of history arrived


@pytest.mark.parametrize("keys", MOVES, ids=lambda k: "+".join(k))
@pytest.mark.parametrize("name,W,H", [("cornell", 65, 49), ("cornell_glass", 40, 33), ("complex", 40, 33),
                                      ("caustic", 40, 33)])
def test_the_fetch_lands_on_the_same_surface_point(name, W, H, keys):
    """Independent of the statement's projection: the history colour is the old view's position / 256
    with weight 1, the frame has no samples, so out = h is the fetched position / 256.  Where all four
    taps were used and the pixel and its (x+1, y+1) neighbour show the same sphere,
    |256 h - P| <= 0.25 |P[y+1, x+1] - P[y, x]|: a mapping off by one pixel puts most pixels above
    that.  At least 35 % of the eligible pixels must qualify for the check."""
    cam0, sp, _, _, aov0 = history_of(name, W, H)
    cam1, _, _, aov1 = case_of(name, W, H, keys)
    hc = (aov0["position"] / F(256)).astype(F)
    hm = np.ones((H, W), F)
    with g.Renderer(sp, W, H, cam1, device=CPU) as r:
        r.history_write(cam0, hc, hm)
        out, w = r.reproject(weight=True)
    zero = np.zeros((H, W), np.uint32)
    _, _, taps = np_reproject(np.zeros((H, W, 3), F), zero, aov1, sp["refl"], hist_dict(cam0, hc, hm, aov0))
    el = eligible(aov1["id"], sp["refl"], "diffuse")
    P = aov1["position"].astype(np.float64)
    check = np.zeros((H, W), bool)
    check[:-1, :-1] = (taps[:-1, :-1] == 4) & el[:-1, :-1] & (aov1["id"][:-1, :-1] == aov1["id"][1:, 1:])
    err = np.linalg.norm(256.0 * out.astype(np.float64) - P, axis=-1)[:-1, :-1]
    step = np.linalg.norm(P[1:, 1:] - P[:-1, :-1], axis=-1)
    with np.errstate(all="ignore"):                            # 0 / 0 between two misses: not checked
        ratio = (err / step)[check[:-1, :-1]]
    share = check.sum() / el.sum()
    print(f"{name} {keys}: checked {check.sum()} of {el.sum()} eligible ({share:.2f}), max ratio {ratio.max():.3f}")
    assert share >= 0.35
    assert (ratio <= 0.25).all(), float(ratio.max())


def test_what_the_validation_rejects():
    name, W, H = "cornell", 65, 49
    cam0, sp, hc, hm, aov0 = history_of(name, W, H)
    keys = KEYSETS[-1]
    cam1, col, cnt, aov1 = case_of(name, W, H, keys)
    with g.Renderer(sp, W, H, cam1, device=CPU) as r:
        r.write_radiance(col, cnt)
        r.history_write(cam0, hc, hm)
        for materials in ("diffuse", "all"):
            out, w = r.reproject(weight=True, materials=materials)
            none = w == cnt.astype(F)
            assert none.any() and (~none).any()
            same(out[none], col[none], "no history taken: the input, bit for bit")
            el = eligible(aov1["id"], sp["refl"], materials)
            assert (~el).any() or materials == "all"
            same(out[~el], col[~el], "ineligible pixels are the input")
            assert none[~el].all()
        # a sphere moved after the history was taken: absent, and the input comes back
        assert r.history_info()[0] is True
        sp2 = sp.copy()
        assert g.sphere_key(sp2, 2, "4")
        r.set_scene(sp2)
        present, c0 = r.history_info()
        assert present is False and bytes(c0) == bytes(cam0)
        out, w = r.reproject(weight=True)
        same(out, col, "scene changed: out == colors")
        same(w, cnt.astype(F), "scene changed: weight == counter")
        r.set_scene(sp)                                        # the same bytes again: present again
        assert r.history_info()[0] is True
        assert (r.reproject(weight=True)[1] != cnt.astype(F)).any()
    cam_m, sp_m = scene("caustic", 40, 33)
    aov_m = first_hit(sp_m, 40, 33, cam_m)
    miss = aov_m["id"] < 0
    assert miss.any()
    colm = synthetic_radiance(40, 33)
    with g.Renderer(sp_m, 40, 33, cam_m, device=CPU) as r:
        r.write_radiance(colm, np.full((33, 40), 2, np.uint32))
        r.history_write(cam_m, synthetic_radiance(40, 33, seed=9), np.full((33, 40), 8, F))
        out, w = r.reproject(weight=True, materials="all", plane_tol=INF)
        same(out[miss], colm[miss], "misses are the input")
        assert (w[miss] == 2).all() and (w[~miss] > 2).any()


def test_rgba_is_the_thresholds_applied_to_the_colours():
    name, W, H = "cornell", 65, 49
    cam0, sp, hc, hm, _ = history_of(name, W, H)
    cam1, col, cnt, _ = case_of(name, W, H, ("left",))
    with g.Renderer(sp, W, H, cam1, device=CPU) as r:
        r.write_radiance(col, cnt)
        r.history_write(cam0, hc, hm)
        out, w, px = r.reproject(weight=True, pixels=True)
        same(out, r.reproject(), "with and without pixels")
        assert px.dtype == np.uint8 and np.array_equal(px, to_rgba(out))
        assert np.array_equal(r.reproject(pixels=True)[1], px)
        assert np.array_equal(r.read_pixels(), to_rgba(col))             # the context's own pixels: untouched
    assert len(np.unique(px[..., :3])) > 50 and not px[..., 3].any()
    assert not np.array_equal(px, to_rgba(col))


def test_errors():
    assert_errors(CPU)


def test_passes_after_capture_and_reproject_equal_passes_without_them():
    assert_non_interference(CPU, "cornell_glass", 33, 25)


@pytest.mark.parametrize("keys", [("left",), ("a",)], ids=lambda k: "+".join(k))
def test_preview_after_a_camera_key_is_closer_to_the_converged_frame(keys):
    """Cornell 65x49 on the CPU backend: 16 passes, capture, the key, ReInit's reset and one pass;
    260 passes of the new view as the truth.  RMSE over all channels of the values clipped to [0, 1]:
    the preview must be at <= 0.7 x the raw frame's (the prototype measured 0.41 for `left`, 0.54 for
    `a`)."""
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
        raw, cnt1 = r.read_radiance()
        assert (cnt1 == 1).all()
        preview = r.reproject()
        r.path_passes(*sched.next(3))
        for _ in range(4):
            r.path_passes(*sched.next(64))
        ref, cnt = r.read_radiance()
    assert (cnt == 260).all()

    def rmse(a):
        d = np.clip(a.astype(np.float64), 0, 1) - np.clip(ref.astype(np.float64), 0, 1)
        return float(np.sqrt((d * d).mean()))

    e_raw, e_prev = rmse(raw), rmse(preview)
    print(f"{keys}: RMSE vs 260 passes: raw {e_raw:.4f}, preview {e_prev:.4f}, ratio {e_prev / e_raw:.3f}")
    assert e_prev <= 0.7 * e_raw, (e_raw, e_prev)


KEYS = ["a", "left", "w", "up", " "]


def _run_keys(app):
    app.IdleFunc()
    app.IdleFunc(3)
    for k in KEYS:
        (app.SpecialFunc if len(k) > 1 else app.KeyFunc)(k)
        app.IdleFunc(2)


def test_the_mirror_without_reuse_history_makes_no_history_call(monkeypatch):
    def forbidden(*a, **k):
        raise AssertionError("history call with reuse_history=False")
    for fn in ("bdpt_history_capture", "bdpt_history_clear", "bdpt_history_write", "bdpt_reproject"):
        monkeypatch.setattr(g.lib, fn, forbidden)
    app = g.SmallPT(20, 19, os.path.join(SCENES, "cornell.scn"), device=CPU)
    assert app.reuse_history is False
    _run_keys(app)
    app.KeyFunc("4")
    app.KeyFunc("+")
    assert app.renderer.history_info() == (False, None)
    app.FreeBuffers()


def test_the_mirror_with_reuse_history_renders_the_same_frame():
    scn = os.path.join(SCENES, "cornell.scn")
    plain, reuse = g.SmallPT(20, 19, scn, device=CPU), g.SmallPT(20, 19, scn, device=CPU, reuse_history=True)
    _run_keys(plain)
    _run_keys(reuse)
    (c0, n0), (c1, n1) = plain.colors(), reuse.colors()
    same(c1, c0, "colors() with and without reuse_history")
    assert np.array_equal(n0, n1) and np.array_equal(plain.pixels(), reuse.pixels())
    present, cam = reuse.renderer.history_info()
    assert present and cam is not None
    prev, w = reuse.preview(weight=True)
    assert (w > n1).any()                                      # and the preview holds more than the frame
    same(plain.preview(), c0, "without a history the preview is the raw frame")
    reuse.KeyFunc("4")                                         # a sphere key: ReInitScene clears
    assert reuse.renderer.history_info()[0] is False
    plain.FreeBuffers()
    reuse.FreeBuffers()


def test_save_preview_ppm_name_and_bytes(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    app = g.SmallPT(20, 19, os.path.join(SCENES, "cornell.scn"), device=CPU, reuse_history=True)
    _run_keys(app)
    raw = app.SavePPM()
    path = app.SavePreviewPPM()
    assert path == raw[:-4] + "_preview.ppm" and os.path.exists(path)
    want = str(tmp_path / "want.ppm")
    g.save_ppm(want, app.renderer.reproject(pixels=True)[1])
    assert open(path, "rb").read() == open(want, "rb").read()
    assert open(path, "rb").read() != open(raw, "rb").read()
    p2 = app.SavePreviewPPM(str(tmp_path / "two.ppm"), binary=True, max_history=2.0, materials="all")
    g.save_ppm(want, app.renderer.reproject(pixels=True, max_history=2.0, materials="all")[1], binary=True)
    assert open(p2, "rb").read() == open(want, "rb").read()
    app.FreeBuffers()


def test_command_line_writes_the_preview(tmp_path):
    """smallpt 20 19 cornell.scn --spp 4 --keys aL --device -1 --reproject --out x.ppm == SavePreviewPPM
    of the mirror driven through the same keys and passes; the options reach the blend."""
    exe = os.path.join(REPO, "gpu_bidirectional_raytracer_amd", "smallpt")
    scn = os.path.join(SCENES, "cornell.scn")
    app = g.SmallPT(20, 19, scn, device=CPU, reuse_history=True)
    app.IdleFunc()
    app.IdleFunc(3)
    app.KeyFunc("a")
    app.IdleFunc(4)
    app.SpecialFunc("left")
    app.IdleFunc(4)
    out, want = str(tmp_path / "x.ppm"), str(tmp_path / "want.ppm")
    base = [exe, "20", "19", scn, "--spp", "4", "--keys", "aL", "--device", "-1", "--dat", g.DEFAULT_DAT, "--out", out]
    # the mirror captured with the defaults; --reproject-history caps each capture and the final blend
    subprocess.run(base + ["--reproject"], check=True, cwd=REPO, capture_output=True, timeout=120)
    app.SavePreviewPPM(want)
    assert open(out, "rb").read() == open(want, "rb").read()
    raw = str(tmp_path / "raw.ppm")
    app.SavePPM(raw)
    assert open(out, "rb").read() != open(raw, "rb").read()             # not the raw frame
    subprocess.run(base, check=True, cwd=REPO, capture_output=True, timeout=120)
    assert open(out, "rb").read() == open(raw, "rb").read()             # without --reproject: unchanged
    app.FreeBuffers()
    # options: a mirror whose captures and preview use them
    app = g.SmallPT(20, 19, scn, device=CPU)
    app.IdleFunc()
    app.IdleFunc(3)
    prm = dict(max_history=2.0, plane_tol=0.5)
    for k in ("a", "left"):
        assert g.camera_key(app.camera, k)
        app.renderer.history_capture(**prm)
        app.ReInit(True)
        app.IdleFunc(4)
    app.SavePreviewPPM(want, **prm)
    subprocess.run(base + ["--reproject", "--reproject-history", "2", "--reproject-tol", "0.5"], check=True, cwd=REPO,
                   capture_output=True, timeout=120)
    assert open(out, "rb").read() == open(want, "rb").read()
    app.FreeBuffers()
    r = subprocess.run(base + ["--reproject", "--gpus", "2"], cwd=REPO, capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "--reproject needs one device" in r.stderr
