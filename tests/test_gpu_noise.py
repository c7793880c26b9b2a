"""The per-tile noise estimate on the GPU (bdpt_noise_kernel and bdpt_noise_mark_kernel,
csrc/bdpt_frame_kernels.h) against the CPU backend -- which tests/test_noise_cpu.py holds to the numpy
statement of the definition -- and against that statement directly.  Every comparison is on the
bits; no tolerance anywhere.  No frame is larger than 65x49; 33x9, 65x49, 40x33, 7x5 and 129x3 are
no multiples of the 32x8 tile, so their launches have partial tiles, 32x8 is exactly one workgroup,
all others but 7x5 more than one."""
import os

import numpy as np
import pytest

import gpu_bidirectional_raytracer_amd as g
from aov_common import same, scene
from conftest import SCENES
from noise_common import (CPU, F, FRAMES, PARAMS, assert_errors, big_case, case, np_noise, run_arrays, run_case,
                          same_estimate, same_summary, want_case)

pytestmark = pytest.mark.gpu

SCN = os.path.join(SCENES, "cornell.scn")


@pytest.mark.parametrize("remark", [False, True], ids=["plain", "remark"])
@pytest.mark.parametrize("W,H", FRAMES, ids=lambda v: str(v))
def test_gpu_equals_cpu_backend(gpu, W, H, remark):
    for prm in PARAMS:
        same_estimate(run_case(gpu, W, H, remark, **prm), run_case(CPU, W, H, remark, **prm), f"{W}x{H} {prm}")


@pytest.mark.parametrize("remark", [False, True], ids=["plain", "remark"])
def test_gpu_equals_the_numpy_definition(gpu, remark):
    same_estimate(run_case(gpu, 65, 49, remark), want_case(65, 49, remark), "65x49")


@pytest.mark.parametrize("remark", [False, True], ids=["plain", "remark"])
def test_counts_near_two_to_the_32(gpu, remark):
    """The kernel forms the integer rules without 64-bit arithmetic; the statement uses int64."""
    col, cnt, mc, mn = big_case()
    got = run_arrays(gpu, col, cnt, mc, mn, remark)
    same_estimate(got, run_arrays(CPU, col, cnt, mc, mn, remark), "counts near 2^32: CPU backend")
    same_estimate(got, np_noise(col, cnt, mc, mn, remark=remark), "counts near 2^32: statement")


def test_error_codes(gpu):
    assert_errors(gpu)
    cam, sp = scene("cornell", 33, 9)
    with g.Renderer(sp, 33, 9, cam, devices=[gpu, gpu]) as r:       # a multi-device context keeps no mark
        for call in (r.noise_mark, r.noise_clear, r.noise_estimate, r.noise_read_mark, r.noise_tiles):
            with pytest.raises(g.BdptError) as ei:
                call()
            assert ei.value.code == g._lib.BDPT_EINVAL


@pytest.mark.parametrize("call", ["reset_accum", "set_scene", "set_camera", "write_radiance", "noise_clear"])
def test_clearing_and_the_mark_that_follows(gpu, call):
    """Each clearing call leaves no valid pixel; the mark taken by the next estimate with remark is
    the CPU backend's (a cleared record keeps its colour and reads the count 0)."""
    W, H = 40, 33
    col, cnt, mc, mn = case(W, H)
    cam, sp = scene("cornell", W, H)
    out = {}
    for dev in (gpu, CPU):
        with g.Renderer(sp, W, H, cam, device=dev) as r:
            r.write_radiance(col, cnt)
            r.noise_write_mark(mc, mn)
            assert r.noise_estimate()["valid_pixels"] > 0
            if call == "set_scene":
                r.set_scene(sp)
            elif call == "set_camera":
                r.set_camera(cam)
            elif call == "write_radiance":
                r.write_radiance(col, cnt)
            else:
                getattr(r, call)()
            if call == "reset_accum":
                r.write_radiance(col, cnt)
            cleared = r.noise_read_mark()
            assert not cleared[1].any()
            first = r.noise_estimate(remark=True, pixels=True)
            assert first["valid_pixels"] == 0
            first["mark"] = r.noise_read_mark()
            out[dev] = (cleared, first)
    same(out[gpu][0][0], out[CPU][0][0], f"{call}: the cleared mark's colours")
    same_estimate(out[gpu][1], out[CPU][1], f"{call}: the estimate that takes the first mark")
    want = np_noise(col, cnt, mc, np.zeros_like(mn), remark=True)
    same_estimate(out[gpu][1], want, f"{call}: against the statement")


def test_frames_of_the_gpus_own_path_kernels(gpu):
    """cornell 65x49: 4 passes, mark, 4 passes, estimate with remark, 8 more, estimate == the numpy
    statement applied twice to the frames read back; the passes rendered equal those of a context
    that never called a noise function; the kernel's time is reported."""
    app, ref = g.SmallPT(64, 48, SCN, device=gpu), g.SmallPT(64, 48, SCN, device=gpu)
    try:
        app.IdleFunc(4)
        ref.IdleFunc(4)
        col4, cnt4 = app.colors()
        app.renderer.noise_mark()
        m = app.renderer.noise_read_mark()
        same(m[0], col4, "noise_mark: colours")
        same(m[1], cnt4, "noise_mark: counts")
        app.IdleFunc(4)
        ref.IdleFunc(4)
        col8, cnt8 = app.colors()
        got1 = app.renderer.noise_estimate(remark=True, pixels=True)
        got1["mark"] = app.renderer.noise_read_mark()
        assert app.renderer.last_noise_ms() > 0
        want1 = np_noise(col8, cnt8, col4, cnt4, remark=True)
        same_estimate(got1, want1, "8 passes against the mark at 4")
        assert got1["valid_pixels"] == 65 * 49 and (want1["mark"][1] == 8).all()
        app.IdleFunc(8)
        ref.IdleFunc(8)
        col16, cnt16 = app.colors()
        got2 = app.renderer.noise_estimate(pixels=True)
        got2["mark"] = app.renderer.noise_read_mark()
        want2 = np_noise(col16, cnt16, *want1["mark"])
        same_estimate(got2, want2, "16 passes against the mark at 8")
        assert got2["valid_pixels"] == 65 * 49 and 0 < got2["mean"] < got1["mean"] * 2
        rc, rn = ref.colors()
        same(col16, rc, "non-interference: colours")
        same(cnt16, rn, "non-interference: counters")
        assert np.array_equal(app.pixels(), ref.pixels())
    finally:
        app.FreeBuffers()
        ref.FreeBuffers()


def test_render_until_stops_where_the_cpu_backend_stops(gpu):
    """The frames are the same bits on both backends, so RenderUntil stops at the same pass with the
    same summary."""
    out = {}
    for dev in (gpu, CPU):
        app = g.SmallPT(64, 48, SCN, device=dev)
        try:
            out[dev] = app.RenderUntil(0.05, max_passes=1024, batch=8)
        finally:
            app.FreeBuffers()
    assert out[gpu]["passes"] == out[CPU]["passes"] and out[gpu]["converged"] == out[CPU]["converged"]
    same_summary(out[gpu], out[CPU], "RenderUntil")
    same(out[gpu]["tile_error"], out[CPU]["tile_error"], "RenderUntil: tile_error")
    same(out[gpu]["tile_valid"], out[CPU]["tile_valid"], "RenderUntil: tile_valid")
    assert out[gpu]["converged"] and out[gpu]["passes"] < 1024
