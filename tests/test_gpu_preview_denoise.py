"""The denoised preview on the GPU (bdpt_reproject_kernel writing the denoiser's records, then
bdpt_preview_level_t / bdpt_preview_level_lds_t, csrc/bdpt_frame_kernels.h) against the CPU backend --
which tests/test_preview_denoise_cpu.py holds to the numpy statement of the definition -- and
against that statement and the existing calls directly.  Every comparison is on the float bits; no
tolerance anywhere.  No frame is larger than 65x49; 65x49, 40x33, 7x5 and 129x3 are no multiples of
the wave or workgroup tiles, so every launch has partial tiles, all but 7x5 more than one workgroup.
Both wave tiles run, with LDS staging on and off (steps 1 and 2 staged, later steps direct, so every
run with more than two levels takes both kernels), whichever of them is the default."""
import ctypes

import numpy as np
import pytest

import gpu_bidirectional_raytracer_amd as g
from aov_common import same, scene
from preview_common import (CPU, F, FRAMES, MOVES, SYNTHETIC_PARAMS, assert_errors, assert_identity_with_denoise,
                            assert_levels0_is_reproject, assert_non_interference, case_of, first_hit, hist_dict,
                            history_of, moved, np_preview_denoise, params_of, results, same_up_to_nan_payload,
                            synthetic_input_is_finite, synthetic_results, to_rgba)

pytestmark = pytest.mark.gpu

VARIANTS = [("64", "1"), ("64", "0"), ("8", "1"), ("8", "0")]     # BDPT_DENOISE_TILE, BDPT_DENOISE_LDS


def _variant(monkeypatch, tile, lds):
    monkeypatch.setenv("BDPT_DENOISE_TILE", tile)
    monkeypatch.setenv("BDPT_DENOISE_LDS", lds)
    monkeypatch.setenv("BDPT_REPROJECT_TILE", tile)


@pytest.fixture(scope="module")
def cpu_results():
    """The CPU backend's results per (frame, keys), computed once, read by every variant, never
    modified."""
    out = {}
    for name, W, H, _ in FRAMES:
        for keys in MOVES:
            if (name, W, H, keys) not in out:
                out[(name, W, H, keys)] = results(CPU, name, W, H, None, keys)
    return out


@pytest.fixture(scope="module")
def cpu_synthetic():
    return synthetic_results(CPU)


# ---- A. the statement -------------------------------------------------------------------------
@pytest.mark.parametrize("tile,lds", VARIANTS)
@pytest.mark.parametrize("name,W,H,traversal", FRAMES)
def test_gpu_equals_cpu_backend(gpu, cpu_results, monkeypatch, name, W, H, traversal, tile, lds):
    _variant(monkeypatch, tile, lds)
    for keys in MOVES:
        got = results(gpu, name, W, H, traversal, keys)
        for prm, (a, aw, ap), (b, bw, bp) in zip(params_of(W, H), got, cpu_results[(name, W, H, keys)]):
            what = f"{name} {W}x{H} {traversal} tile {tile} lds {lds} {keys} {prm}"
            same(a, b, what + ": colours")
            same(aw, bw, what + ": count")
            assert np.array_equal(ap, bp), what


@pytest.mark.parametrize("tile,lds", VARIANTS)
def test_synthetic_history_with_holes_and_absurd_weights(gpu, cpu_synthetic, monkeypatch, tile, lds):
    """History colours with 0, -0, 1e-30 and 1e18, weights 0, 1e-30, 0.5, 1, 64, 3e4 and 1e30 in
    blocks, from a reset accumulation (holes next to filled pixels: the a_p == 0 branch) and after
    one pass: GPU == CPU backend, which the CPU test holds to the statement."""
    _variant(monkeypatch, tile, lds)
    got = synthetic_results(gpu)
    finite = synthetic_input_is_finite()
    assert all(finite[0]) and sum(finite[1]) >= 1
    for state, (gs, cs) in enumerate(zip(got, cpu_synthetic)):
        for k, (prm, (a, aw, ap), (b, bw, bp)) in enumerate(zip(SYNTHETIC_PARAMS, gs, cs)):
            what = f"synthetic, state {state}, tile {tile} lds {lds} {prm}"
            # a frame that bdpt_reproject's blend has already overflowed (preview_common) breeds
            # NaNs, whose sign and payload IEEE 754 leaves open: there a NaN equals any NaN
            eq = same if finite[state][k] else same_up_to_nan_payload
            eq(a, b, what + ": colours")
            eq(aw, bw, what + ": count")
            assert np.array_equal(ap, bp), what
    w0 = got[0][0][1]
    assert (w0 == 0).any() and (w0 > 0).any()


def test_default_variant_on_frames_rendered_on_the_gpu(gpu):
    """No environment override; history and frame rendered by the GPU's own path kernels and captured
    on the GPU, a window of feature buffers asked for first (so the planes have to grow): equal to
    the numpy statement, colours, count and pixels, and each output alone equals the joint call."""
    name, W, H = "cornell", 65, 49
    cam0, sp = scene(name, W, H)
    cam1 = moved(cam0, ("a",), W, H)
    sched = g.PassScheduler()
    with g.Renderer(sp, W, H, cam0, device=gpu) as r:
        r.light_pass(0)
        sched.light()
        r.path_passes(*sched.next(4))
        colA, cntA = r.read_radiance()
        r.render_aov(window=(3, 2, 9, 5))
        r.history_capture()
        r.reset_accum()
        r.set_camera(cam1)
        r.path_passes(*sched.next(1))
        colB, cntB = r.read_radiance()
        got, gw, px = r.preview_denoise(weight=True, pixels=True)
        assert r.last_preview_ms() > 0.0
        same(r.preview_denoise(), got, "with and without weight and pixels")
        only_px, only_w = np.empty((H, W, 4), np.uint8), np.empty((H, W), F)
        prm = g._lib.PreviewParams(g._lib.ReprojectParams(0, 64.0, 0.01), 4, 5, 0.5, 8.0)
        assert g.lib.bdpt_preview_denoise(r._h, ctypes.byref(prm), None, None, ctypes.c_void_p(only_px.ctypes.data)) == 0
        assert g.lib.bdpt_preview_denoise(r._h, ctypes.byref(prm), None, ctypes.c_void_p(only_w.ctypes.data), None) == 0
        assert np.array_equal(only_px, px)
        same(only_w, gw, "count alone")
        assert np.array_equal(r.read_pixels(), to_rgba(colB))               # the context's own pixels: untouched
        # the existing calls after it, on the buffers it shares with them
        same(r.reproject(), r.preview_denoise(levels=0), "reproject() after the call")
    aov0, aov1 = first_hit(sp, W, H, cam0, gpu), first_hit(sp, W, H, cam1, gpu)
    o, a, tot = np_preview_denoise(colB, cntB, aov1, sp["refl"], hist_dict(cam0, colA, cntA.astype(F), aov0))
    same(got, o, "GPU vs numpy: colours")
    same(gw, a, "GPU vs numpy: count")
    assert np.array_equal(px, to_rgba(o))
    assert (tot > 4).any() and (tot == 1).any() and (a != tot).any()


# ---- B. ties to the code that exists ----------------------------------------------------------
@pytest.mark.parametrize("tile", ["64", "8"])
def test_levels_0_is_reproject(gpu, monkeypatch, tile):
    monkeypatch.setenv("BDPT_REPROJECT_TILE", tile)
    assert_levels0_is_reproject(gpu, "cornell", 65, 49, ("left",))
    assert_levels0_is_reproject(gpu, "caustic", 40, 33, ("a",))


@pytest.mark.parametrize("tile,lds", VARIANTS)
@pytest.mark.parametrize("name,W,H", [("cornell", 33, 25), ("cornell_glass", 65, 49)])
def test_uniform_eight_passes_without_history_is_denoise(gpu, monkeypatch, name, W, H, tile, lds):
    _variant(monkeypatch, tile, lds)
    assert_identity_with_denoise(gpu, name, W, H)


# ---- E. non-interference ----------------------------------------------------------------------
@pytest.mark.parametrize("streams", [0, 1])
def test_passes_after_the_call_equal_passes_without_it(gpu, streams):
    assert_non_interference(gpu, "cornell_glass", 65, 49, streams=streams)


# ---- F. errors --------------------------------------------------------------------------------
def test_errors(gpu):
    assert_errors(gpu)
    cam, sp = scene("cornell", 20, 19)
    with g.Renderer(sp, 20, 19, cam, devices=[gpu, gpu]) as r:          # a multi-device context
        with pytest.raises(g.BdptError) as e:
            r.preview_denoise()
        assert e.value.code == g._lib.BDPT_EINVAL
        with pytest.raises(g.BdptError) as e:
            r.last_preview_ms()
        assert e.value.code == g._lib.BDPT_ESTATE
