"""The noise-guided denoiser on the GPU (bdpt_dnoise_pack_kernel, bdpt_dnoise_prefilter_kernel and the
level kernels' third mode, csrc/bdpt_frame_kernels.h) against the numpy statement of the definition
(tests/denoise_noise_common.py) -- which tests/test_denoise_noise_cpu.py holds the CPU backend to --
and against that backend.  Every comparison is on the float bits; no tolerance anywhere.  7x5 lies
inside one tile and outside the later levels' steps; 33x25, 40x33 and 65x49 are no multiples of the
8x8 / 64x1 wave tiles or the 32x8 / 64x4 workgroup tiles, so every launch has partial tiles and
taps across tile and halo borders of the prefilter and of both level kernels.  Both tile shapes
and the LDS-staged level kernel are run, whichever of them is the default."""
import numpy as np
import pytest

import gpu_bidirectional_raytracer_amd as g
from aov_common import same, scene
from denoise_common import FRAMES
from denoise_noise_common import (CPU, SWEEP, SYNTHETIC, assert_equals_plain_denoise, assert_errors,
                                  assert_matches_numpy, assert_non_interference, assert_render_until,
                                  assert_zero_variance_passes_through, big_case, case, guides, raw_variance,
                                  rendered_marked, run)

pytestmark = pytest.mark.gpu

# (BDPT_DENOISE_TILE, BDPT_DENOISE_LDS): the kernel variants of csrc/bdpt_frame.cpp run_levels
VARIANTS = [("8", "0"), ("64", "0"), ("8", "1"), ("64", "1")]


@pytest.fixture(scope="module")
def rendered():
    """Per frame: the 4 + 4-pass radiance with the mark between, from the CPU backend (bit-identical
    to the GPU's path kernels by the project's other tests); computed once, never modified."""
    return {(n, W, H): rendered_marked(CPU, n, W, H) for n, W, H in FRAMES}


@pytest.mark.parametrize("name,W,H", FRAMES, ids=lambda v: str(v))
def test_rendered_frames_equal_the_numpy_definition(gpu, rendered, name, W, H):
    cam, sp, col, cnt, mark = rendered[(name, W, H)]
    with g.Renderer(sp, W, H, cam, device=gpu) as r:
        r.write_radiance(col, cnt)
        r.noise_write_mark(*mark)
        aov = r.render_aov()
        assert_matches_numpy(r, col, cnt, mark, aov["id"], aov["normal"], sp["refl"], f"{name} {W}x{H}")
        same(r.read_radiance()[0], col, "the accumulation is only read")
        same(r.noise_read_mark()[1], mark[1], "the mark is only read")
        assert r.last_denoise_noise_ms() > 0.0


@pytest.mark.parametrize("tile,lds", VARIANTS)
@pytest.mark.parametrize("name,W,H", SYNTHETIC, ids=lambda v: str(v))
def test_synthetic_frames_equal_the_cpu_backend(gpu, monkeypatch, name, W, H, tile, lds):
    """Every kernel variant on frames whose pixels with and without an estimate sit next to each
    other (values 0, -0, 1e-30 and 1e18, counts 0 .. 30000)."""
    monkeypatch.setenv("BDPT_DENOISE_TILE", tile)
    monkeypatch.setenv("BDPT_DENOISE_LDS", lds)
    col, cnt, mc, mn = case(W, H)
    cam, sp = scene(name, W, H)
    res = []
    for dev in (CPU, gpu):
        with g.Renderer(sp, W, H, cam, device=dev) as r:
            r.write_radiance(col, cnt)
            r.noise_write_mark(mc, mn)
            res.append([run(r, **prm) for prm in SWEEP[::3] + SWEEP[1::7]])
            if dev == gpu:
                for a, b in zip(run(r, **SWEEP[1]), res[-1][len(SWEEP[::3])]):
                    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), "a second call"
    for want, got in zip(*res):
        for a, b, what in zip(want, got, ("colours", "pixels", "variance")):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"{W}x{H} tile {tile} lds {lds}: {what}"


def test_default_variant_on_synthetic_frames_vs_numpy(gpu):
    for name, W, H in SYNTHETIC:
        col, cnt, mc, mn = case(W, H)
        cam, sp, ids, nrm = guides(name, W, H)
        with g.Renderer(sp, W, H, cam, device=gpu) as r:
            r.write_radiance(col, cnt)
            r.noise_write_mark(mc, mn)
            assert_matches_numpy(r, col, cnt, (mc, mn), ids, nrm, sp["refl"], f"synthetic {W}x{H}")


def test_counts_near_two_to_the_32(gpu):
    col, cnt, mc, mn = big_case()
    H, W = cnt.shape
    cam, sp, ids, nrm = guides("cornell_glass", W, H)
    v0 = raw_variance(col, cnt, mc, mn)
    assert ((v0 >= 0) & (cnt >= 2 ** 31)).any()
    with g.Renderer(sp, W, H, cam, device=gpu) as r:
        r.write_radiance(col, cnt)
        r.noise_write_mark(mc, mn)
        assert_matches_numpy(r, col, cnt, (mc, mn), ids, nrm, sp["refl"], "counts near 2^32", sweep=SWEEP[6:12])


def test_a_frame_rendered_and_marked_on_the_gpu(gpu):
    """The GPU's own path kernels and bdpt_noise_mark, a window of feature buffers asked for first (so
    the guide planes have to grow), complex's BVH for the guides: equal to the numpy statement."""
    name, W, H = "complex", 40, 33
    cam, sp, col, cnt, mark = rendered_marked(gpu, name, W, H)
    with g.Renderer(sp, W, H, cam, device=gpu) as r:
        r.write_radiance(col, cnt)
        r.noise_write_mark(*mark)
        r.render_aov(window=(3, 2, 9, 5))
        out, px, var = run(r)
        aov = r.render_aov()
    from denoise_noise_common import np_denoise_noise
    want, wvar = np_denoise_noise(col, cnt, mark, aov["id"], aov["normal"], sp["refl"])
    same(out, want, "defaults vs numpy: colours")
    same(var, wvar, "defaults vs numpy: variance")
    assert (var >= 0).any()


def test_without_an_estimate_it_is_the_plain_denoiser(gpu):
    assert_equals_plain_denoise(gpu)


def test_zero_variance_passes_through(gpu):
    assert_zero_variance_passes_through(gpu)


@pytest.mark.parametrize("streams", [0, 1])
def test_passes_after_the_call_equal_passes_without_it(gpu, streams):
    assert_non_interference(gpu, "cornell_glass", 65, 49, streams=streams)


def test_render_until_with_denoise(gpu):
    assert_render_until(gpu)


def test_errors(gpu):
    assert_errors(gpu)
    cam, sp = scene("cornell", 20, 19)
    with g.Renderer(sp, 20, 19, cam, devices=[gpu, gpu]) as r:          # a multi-device context
        with pytest.raises(g.BdptError) as e:
            r.denoise_noise()
        assert e.value.code == g._lib.BDPT_EINVAL
