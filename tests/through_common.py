"""Shared by tests/test_denoise_through_cpu.py and tests/test_gpu_denoise_through.py (not a test
module): materials = "through" of denoise and denoise_noise against the existing numpy models
(tests/denoise_common.py np_denoise, tests/denoise_noise_common.py np_denoise_noise), imported as
they are and fed the chain's guides -- the key and the end normal of the numpy statement of
bdpt_render_chain (tests/chain_common.py; jitter 0, TRANSMIT, whole frame), every key an eligible
id (the models' materials = "all").  Every comparison is on float32 bits; no tolerance."""
import numpy as np
import pytest

import gpu_bidirectional_raytracer_amd as g
from chain_common import cam_floats, guide_keys, np_chain, same, scene
from denoise_common import np_denoise, rendered_frame, to_rgba
from denoise_noise_common import np_denoise_noise, rendered_marked

CPU = -1
MODEL_SCENES = [("cornell_mirror", 33, 25), ("cornell_glass", 33, 25)]
# no mirror and no glass in view -- and no emitter of refl DIFF, which "diffuse" filters and "through"
# (eligible iff the chain ends DIFFUSE, not EMITTER) copies through
PLAIN_SCENES = [("cornell_diff", 33, 25), ("cornell_diff_BL", 33, 25)]


def through_guides(cam, sp, W, H):
    """(keys, end normals, the statement's chain) of the unjittered TRANSMIT chain."""
    chain = np_chain(sp, cam_floats(cam), W, H)
    return guide_keys(chain, len(sp)), chain["normal"], chain


def assert_matches_models(device, name, W, H):
    """denoise with levels 1 and 4 and denoise_noise with a mark at N / 2 (4 of 8 passes), through."""
    cam, sp, col, cnt, mark = rendered_marked(CPU, name, W, H)
    keys, nrm, chain = through_guides(cam, sp, W, H)
    assert (chain["bounces"][keys >= 0] > 0).any(), "no pixel is guided through a mirror or glass"
    with g.Renderer(sp, W, H, cam, device=device) as r:
        r.write_radiance(col, cnt)
        for levels in (1, 4):
            out, px = r.denoise(levels=levels, materials="through", pixels=True)
            same(out, np_denoise(col, keys, nrm, sp["refl"], levels=levels, materials="all"), f"{name} levels {levels}")
            assert np.array_equal(px, to_rgba(out))
        plain = r.denoise_noise(materials="through")                  # no mark yet: denoise's bits
        same(plain, r.denoise(materials="through"), f"{name}: denoise_noise without a mark")
        r.noise_write_mark(*mark)
        out, px, var = r.denoise_noise(materials="through", pixels=True, variance=True)
        want, wvar = np_denoise_noise(col, cnt, mark, keys, nrm, sp["refl"], materials="all")
        same(out, want, f"{name}: denoise_noise colours")
        same(var, wvar, f"{name}: denoise_noise variance")
        assert np.array_equal(px, to_rgba(out))
        assert (np.ascontiguousarray(out).view(np.uint32) != np.ascontiguousarray(plain).view(np.uint32)).any()
        # the mirrors' and the glass's pixels are filtered, which "diffuse" copies through
        raw = r.denoise(materials="diffuse")
        through = r.denoise(materials="through")
        moved = (keys >= 0) & (chain["bounces"] > 0)
        same(raw[moved], col[moved], f"{name}: diffuse leaves them raw")
        assert (through[moved] != col[moved]).any(axis=-1).mean() > 0.9


def assert_plain_scene_equals_diffuse(device, name, W, H):
    """Without a mirror or glass in view every key is the first hit's id: "diffuse"'s bits."""
    cam, sp, col, cnt, mark = rendered_marked(CPU, name, W, H)
    keys, _, chain = through_guides(cam, sp, W, H)
    assert (chain["bounces"] == 0).all()
    with g.Renderer(sp, W, H, cam, device=device) as r:
        r.write_radiance(col, cnt)
        same(r.denoise(materials="through"), r.denoise(materials="diffuse"), f"{name}: denoise")
        r.noise_write_mark(*mark)
        for a, b, what in zip(r.denoise_noise(materials="through", variance=True),
                              r.denoise_noise(materials="diffuse", variance=True), ("colours", "variance")):
            same(a, b, f"{name}: denoise_noise {what}")


def assert_cornell_partition(device):
    """cornell shows a mirror and a glass ball: "through" equals "diffuse" on every pixel whose chain
    has no bounce (their keys are their ids, and no pixel behind a ball shares one), and "diffuse"
    leaves the others raw."""
    W, H = 33, 25
    cam, sp, col, cnt = rendered_frame(CPU, "cornell", W, H)
    _, _, chain = through_guides(cam, sp, W, H)
    direct = chain["bounces"] == 0
    assert 0 < (~direct).sum() < direct.sum()
    with g.Renderer(sp, W, H, cam, device=device) as r:
        r.write_radiance(col, cnt)
        d, t = r.denoise(materials="diffuse"), r.denoise(materials="through")
    same(t[direct], d[direct], "cornell: pixels without a bounce")
    same(d[~direct], col[~direct], "cornell: diffuse copies the balls through")


def assert_refusals(device):
    """reproject, history_capture and preview_denoise refuse the value (BDPT_EINVAL)."""
    cam, sp = scene("cornell_mirror", 20, 19)
    with g.Renderer(sp, 20, 19, cam, device=device) as r:
        r.light_pass(0)
        for call in (lambda: r.reproject(materials="through"), lambda: r.preview_denoise(materials="through"),
                     lambda: r.history_capture(materials="through")):
            with pytest.raises(g.BdptError) as e:
                call()
            assert e.value.code == g._lib.BDPT_EINVAL
        assert r.denoise(materials="through").shape == (19, 20, 3)
