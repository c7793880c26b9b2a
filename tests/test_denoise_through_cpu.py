"""materials = "through" of the denoisers (include/bdpt.h BDPT_DENOISE_THROUGH) on the CPU backend;
runs without a GPU.  Against the existing numpy models fed the chain's guides (tests/through_common.py),
bit for bit; and -- the only tolerance here -- that the filter removes noise behind mirrors and glass
(RMSE against a 260-pass frame)."""
import os
import subprocess

import numpy as np
import pytest

import gpu_bidirectional_raytracer_amd as g
from chain_common import KIND_DIFFUSE, scene
from conftest import REPO, SCENES
from denoise_common import rendered_frame
from through_common import (CPU, MODEL_SCENES, PLAIN_SCENES, assert_cornell_partition, assert_matches_models,
                            assert_plain_scene_equals_diffuse, assert_refusals)


@pytest.fixture(autouse=True)
def threads(monkeypatch):
    monkeypatch.setenv("BDPT_CPU_THREADS", "4")


@pytest.mark.parametrize("name,W,H", MODEL_SCENES)
def test_equals_the_models_fed_chain_guides(name, W, H):
    assert_matches_models(CPU, name, W, H)


@pytest.mark.parametrize("name,W,H", PLAIN_SCENES)
def test_without_specular_spheres_in_view_it_is_diffuse(name, W, H):
    assert_plain_scene_equals_diffuse(CPU, name, W, H)


def test_cornell_differs_only_behind_its_balls():
    assert_cornell_partition(CPU)


def test_reproject_and_preview_refuse_it():
    assert_refusals(CPU)


def test_too_many_spheres_for_the_keys():
    """6 n^2 + n > 2^31 - 1 from n = 18919: BDPT_EINVAL for "through" only; n = 18918 is served."""
    cam, _ = scene("cornell_mirror", 20, 19)
    for n, fits in ((18918, True), (18919, False)):
        assert (6 * n * n + n <= 2 ** 31 - 1) == fits
        sp = np.zeros(n, g.SPHERE_DTYPE)
        sp["rad"] = 0.5
        sp["p"] = np.stack([np.arange(n) * 2.0 + 1e4, np.zeros(n), np.zeros(n)], axis=1)   # a row far off the view
        sp["c"] = 0.5
        sp["p"][0], sp["rad"][0] = (50, 40, 80), 30.0                                     # one sphere in view
        with g.Renderer(sp, 20, 19, cam, device=CPU) as r:
            r.light_pass(0)
            for call in (r.denoise, r.denoise_noise):
                assert call(materials="diffuse").shape == (19, 20, 3)
                if fits:
                    assert call(materials="through").shape == (19, 20, 3)
                else:
                    with pytest.raises(g.BdptError) as e:
                        call(materials="through")
                    assert e.value.code == g._lib.BDPT_EINVAL


def test_through_reduces_the_error_behind_mirrors_and_glass():
    """cornell_mirror 65x49 on the CPU backend with the reference's pass schedule, values clipped to
    [0, 1], against the 260-pass frame.  Over the pixels whose first hit is SPEC or REFR and whose
    chain ends DIFFUSE (1737 of 3185) the 4-pass frame -- which "diffuse" leaves as it is there -- has
    RMSE 0.1349 and "through" 0.0885, ratio 0.656; asserted with the headroom test_denoise_cpu.py
    took (0.671 measured, 0.8 asserted: + 0.129): <= 0.785.  Whole frame: raw 0.1786, "diffuse"
    0.1472, "through" 0.1266."""
    W, H = 65, 49
    cam, sp = scene("cornell_mirror", W, H)
    sched = g.PassScheduler()
    with g.Renderer(sp, W, H, cam, device=CPU) as r:
        r.light_pass(0)
        sched.light()
        r.path_passes(*sched.next(4))
        noisy, _ = r.read_radiance()
        diffuse, through = r.denoise(materials="diffuse"), r.denoise(materials="through")
        chain = r.render_chain()
        for _ in range(4):
            r.path_passes(*sched.next(64))
        ref, cnt = r.read_radiance()
    assert (cnt == 260).all()
    first = sp["refl"][np.where(chain["first_id"] >= 0, chain["first_id"], 0)]
    region = (chain["first_id"] >= 0) & ((first == g.SPEC) | (first == g.REFR)) & (chain["kind"] == KIND_DIFFUSE)
    assert region.sum() > 1000
    assert np.array_equal(diffuse[region], noisy[region])               # the raw frame is what "diffuse" leaves there

    def rmse(a, mask=None):
        d = np.clip(a.astype(np.float64), 0, 1) - np.clip(ref.astype(np.float64), 0, 1)
        d = d[mask] if mask is not None else d
        return float(np.sqrt((d * d).mean()))

    e_raw, e_through = rmse(noisy, region), rmse(through, region)
    print(f"RMSE vs 260 passes behind mirrors and glass ({int(region.sum())} px): raw {e_raw:.4f}, through "
          f"{e_through:.4f}, ratio {e_through / e_raw:.3f}; whole frame: raw {rmse(noisy):.4f}, diffuse "
          f"{rmse(diffuse):.4f}, through {rmse(through):.4f}")
    assert e_through <= 0.785 * e_raw, (e_raw, e_through)
    assert rmse(through) < rmse(diffuse)


def test_front_ends(tmp_path, monkeypatch):
    """smallpt --denoise --denoise-through and SmallPT.SaveDenoisedPPM(materials="through") write
    Renderer.denoise(materials="through")'s pixels."""
    exe = os.path.join(REPO, "gpu_bidirectional_raytracer_amd", "smallpt")
    scn = os.path.join(SCENES, "cornell_mirror.scn")
    cam, sp, col, cnt = rendered_frame(CPU, "cornell_mirror", 21, 20)    # sizes get +1
    out, want = str(tmp_path / "x.ppm"), str(tmp_path / "want.ppm")
    subprocess.run([exe, "20", "19", scn, "--spp", "4", "--device", "-1", "--dat", g.DEFAULT_DAT, "--denoise",
                    "--denoise-through", "--out", out], check=True, cwd=REPO, capture_output=True, timeout=120)
    with g.Renderer(sp, 21, 20, cam, device=CPU) as r:
        r.write_radiance(col, cnt)
        g.save_ppm(want, r.denoise(pixels=True, materials="through")[1])
        assert open(out, "rb").read() == open(want, "rb").read()
        g.save_ppm(want, r.denoise(pixels=True)[1])
        assert open(out, "rb").read() != open(want, "rb").read()
    monkeypatch.chdir(tmp_path)
    app = g.SmallPT(20, 19, scn, device=CPU)
    app.IdleFunc()
    app.IdleFunc(3)
    path = app.SaveDenoisedPPM(materials="through")
    g.save_ppm(want, app.renderer.denoise(pixels=True, materials="through")[1])
    assert open(path, "rb").read() == open(want, "rb").read()
    app.FreeBuffers()
