"""The edge-avoiding wavelet denoiser on the GPU (bdpt_denoise_pack_kernel and the level kernels,
csrc/bdpt_frame_kernels.h) against the CPU backend -- which tests/test_denoise_cpu.py holds to the numpy
statement of the definition -- and against that statement directly.  Every comparison is on the
float bits; no tolerance anywhere.  65x49, 40x33, 7x5 and 129x3 are no multiples of the 8x8 / 64x1
wave tiles or the 32x8 / 64x4 workgroup tiles: every launch has partial tiles, all but 7x5 more than
one workgroup, and step 16 (levels = 5) exceeds half of the small frames.  Both tile shapes and the
LDS-staged level kernel are run, whichever of them is the default."""
import numpy as np
import pytest

import gpu_bidirectional_raytracer_amd as g
from aov_common import same, scene
from denoise_common import (DEFAULTS, FRAMES, SWEEP, assert_errors, assert_non_interference, eligible, np_denoise,
                            rendered_frame, synthetic_radiance, to_rgba)

pytestmark = pytest.mark.gpu

CPU = -1
# (scene, W, H, traversal of the guides)
GPU_FRAMES = [(n, W, H, None) for n, W, H in FRAMES if n != "complex"] + [
    ("complex", 40, 33, "brute"), ("complex", 40, 33, "bvh"), ("cornell", 129, 3, None)]
# (BDPT_DENOISE_TILE, BDPT_DENOISE_LDS): the kernel variants of csrc/bdpt_frame.cpp run_levels
VARIANTS = [("8", "0"), ("64", "0"), ("8", "1"), ("64", "1")]


@pytest.fixture(scope="module")
def cpu_results():
    """Per frame: the 4-pass radiance and the CPU backend's denoised frames over the sweep, computed
    once, read by several tests, never modified."""
    out = {}
    for name, W, H, _ in GPU_FRAMES:
        if (name, W, H) in out:
            continue
        cam, sp, col, cnt = rendered_frame(CPU, name, W, H)
        with g.Renderer(sp, W, H, cam, device=CPU) as r:
            r.write_radiance(col, cnt)
            out[(name, W, H)] = (cam, sp, col, cnt, [r.denoise(**prm) for prm in SWEEP])
    return out


@pytest.mark.parametrize("tile,lds", VARIANTS)
@pytest.mark.parametrize("name,W,H,traversal", GPU_FRAMES)
def test_gpu_equals_cpu_backend(gpu, cpu_results, monkeypatch, name, W, H, traversal, tile, lds):
    monkeypatch.setenv("BDPT_DENOISE_TILE", tile)
    monkeypatch.setenv("BDPT_DENOISE_LDS", lds)
    cam, sp, col, cnt, want = cpu_results[(name, W, H)]
    with g.Renderer(sp, W, H, cam, device=gpu) as r:
        if traversal:
            r.set_traversal(traversal)
        r.write_radiance(col, cnt)
        for prm, ref in zip(SWEEP, want):
            same(r.denoise(**prm), ref, f"{name} {W}x{H} {traversal} tile {tile} lds {lds} {prm}")
        same(r.read_radiance()[0], col, "the accumulation is only read")
        assert r.last_denoise_ms() > 0.0


def test_default_variant_on_a_frame_rendered_on_the_gpu(gpu):
    """No environment override, the frame rendered by the GPU's own path kernels, a window of feature
    buffers asked for first (so the guide planes have to grow): equal to the numpy statement."""
    name, W, H = "cornell_glass", 65, 49
    cam, sp, col, cnt = rendered_frame(gpu, name, W, H)
    with g.Renderer(sp, W, H, cam, device=gpu) as r:
        r.write_radiance(col, cnt)
        r.render_aov(window=(3, 2, 9, 5))
        out = r.denoise()
        aov = r.render_aov()
    same(out, np_denoise(col, aov["id"], aov["normal"], sp["refl"]), "defaults vs numpy")
    el = eligible(aov["id"], sp["refl"], "diffuse")
    same(out[~el], col[~el], "ineligible pixels are the input")
    assert el.any() and (~el).any()


@pytest.mark.parametrize("tile,lds", VARIANTS)
def test_synthetic_radiance_with_underflowing_weights(gpu, monkeypatch, tile, lds):
    monkeypatch.setenv("BDPT_DENOISE_TILE", tile)
    monkeypatch.setenv("BDPT_DENOISE_LDS", lds)
    name, W, H = "cornell_glass", 40, 33
    cam, sp = scene(name, W, H)
    col = synthetic_radiance(W, H)
    cnt = np.full((H, W), 3, np.uint32)
    res = []
    for dev in (CPU, gpu):
        with g.Renderer(sp, W, H, cam, device=dev) as r:
            r.write_radiance(col, cnt)
            res.append([r.denoise(levels=l, normal_power=p, sigma_color=1e-3, materials=m)
                        for m in ("diffuse", "all") for l, p in ((1, 6), (4, 6), (5, 5), (2, 0))])
            if dev == gpu:
                same(r.denoise(levels=2, normal_power=0, sigma_color=1e-3, materials="all"), res[-1][-1],
                     "a second call")
    for a, b in zip(*res):
        same(b, a, f"synthetic radiance, tile {tile} lds {lds}")


def test_rgba_is_the_thresholds_applied_to_the_colours(gpu, cpu_results):
    cam, sp, col, cnt, _ = cpu_results[("cornell_glass", 65, 49)]
    with g.Renderer(sp, 65, 49, cam, device=gpu) as r:
        r.write_radiance(col, cnt)
        for prm in (DEFAULTS, dict(DEFAULTS, materials="all", levels=1)):
            out, px = r.denoise(pixels=True, **prm)
            same(out, r.denoise(**prm), "with and without pixels")
            assert np.array_equal(px, to_rgba(out))
        # pixels alone (no colours wanted) through the C ABI
        import ctypes
        only = np.empty((49, 65, 4), np.uint8)
        prm = g._lib.DenoiseParams(1, 5, 0.5, 1)
        assert g.lib.bdpt_denoise(r._h, ctypes.byref(prm), None, ctypes.c_void_p(only.ctypes.data)) == 0
        assert np.array_equal(only, px)
        assert np.array_equal(r.read_pixels(), to_rgba(col))             # the context's own pixels: untouched


@pytest.mark.parametrize("streams", [0, 1])
def test_passes_after_denoise_equal_passes_without_it(gpu, streams):
    assert_non_interference(gpu, "cornell_glass", 65, 49, streams=streams)


def test_errors(gpu):
    assert_errors(gpu)
    cam, sp = scene("cornell", 20, 19)
    with g.Renderer(sp, 20, 19, cam, devices=[gpu, gpu]) as r:          # a multi-device context
        with pytest.raises(g.BdptError) as e:
            r.denoise()
        assert e.value.code == g._lib.BDPT_EINVAL
