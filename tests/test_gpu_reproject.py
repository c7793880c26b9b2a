"""Temporal reprojection on the GPU (bdpt_history_pack_kernel and bdpt_reproject_kernel,
csrc/bdpt_frame_kernels.h) against the CPU backend -- which tests/test_reproject_cpu.py holds to the numpy
statement of the definition -- and against that statement directly.  Every comparison is on the
float bits; no tolerance anywhere.  65x49, 40x33, 7x5 and 129x3 are no multiples of the 8x8 / 64x1
wave tiles or the 32x8 / 64x4 workgroup tiles: every launch has partial tiles, all but 7x5 more than
one workgroup.  Both wave tiles are run, whichever of them is the default."""
import ctypes

import numpy as np
import pytest

import gpu_bidirectional_raytracer_amd as g
from aov_common import same, scene
from reproject_common import (CPU, F, FRAMES, INF, KEYSETS, MOVES, SWEEP, assert_errors, assert_non_interference,
                              case_of, first_hit, hist_dict, history_of, moved, np_reproject, patterned_weight,
                              synthetic_radiance, to_rgba)

pytestmark = pytest.mark.gpu

TILES = ["64", "8"]                                      # BDPT_REPROJECT_TILE


def _results(device, name, W, H, traversal, keys, hm=None):
    """reproject (out, weight) and the capture's history_read over the sweep, history written under the
    old camera and a one-pass frame under the new one (both rendered once on the CPU backend)."""
    cam0, sp, hc, hm4, _ = history_of(name, W, H)
    hm = hm4 if hm is None else hm
    cam1, col, cnt, _ = case_of(name, W, H, keys)
    res = []
    with g.Renderer(sp, W, H, cam1, device=device) as r:
        if traversal and device != CPU:
            r.set_traversal(traversal)
        r.write_radiance(col, cnt)
        for prm in SWEEP:
            r.history_write(cam0, hc, hm)
            res.append(r.reproject(weight=True, **prm))
            r.history_capture(**prm)
            res.append(r.history_read())
        same(r.read_radiance()[0], col, "the accumulation is only read")
        if device != CPU:
            assert r.last_reproject_ms() > 0.0
    return res


@pytest.fixture(scope="module")
def cpu_results():
    """The CPU backend's results per (frame, keys), computed once, read by both tile variants, never
    modified."""
    out = {}
    for name, W, H, _ in FRAMES:
        for keys in KEYSETS:
            if (name, W, H, keys) not in out:
                out[(name, W, H, keys)] = _results(CPU, name, W, H, None, keys)
    return out


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("name,W,H,traversal", FRAMES)
def test_gpu_equals_cpu_backend(gpu, cpu_results, monkeypatch, name, W, H, traversal, tile):
    monkeypatch.setenv("BDPT_REPROJECT_TILE", tile)
    for keys in KEYSETS:
        got = _results(gpu, name, W, H, traversal, keys)
        for k, ((a, aw), (b, bw)) in enumerate(zip(got, cpu_results[(name, W, H, keys)])):
            what = f"{name} {W}x{H} {traversal} tile {tile} {keys} {SWEEP[k // 2]} {'capture' if k % 2 else 'reproject'}"
            same(a, b, what + ": colours")
            same(aw, bw, what + ": weight")


@pytest.mark.parametrize("tile", TILES)
def test_uneven_history_and_synthetic_radiance(gpu, monkeypatch, tile):
    """A different history count per pixel (zeros included), seeded radiance with 0, -0, 1e-30 and
    1e18 on both sides, counters 0..3: GPU == CPU backend."""
    monkeypatch.setenv("BDPT_REPROJECT_TILE", tile)
    name, W, H = "cornell_glass", 40, 33
    cam0, sp = scene(name, W, H)
    hc, col, hm = synthetic_radiance(W, H), synthetic_radiance(W, H, seed=7), patterned_weight(W, H)
    y, x = np.mgrid[0:H, 0:W]
    cnt = ((x + 2 * y) % 4).astype(np.uint32)
    for keys in MOVES[:2]:
        cam1 = moved(cam0, keys, W, H)
        res = []
        for dev in (CPU, gpu):
            with g.Renderer(sp, W, H, cam1, device=dev) as r:
                r.write_radiance(col, cnt)
                r.history_write(cam0, hc, hm)
                same(r.history_read()[0], hc, "history_read after history_write: colours")
                same(r.history_read()[1], hm, "history_read after history_write: weight")
                res.append([r.reproject(weight=True, materials=m, max_history=mh, plane_tol=tol)
                            for m in ("diffuse", "all") for mh, tol in ((INF, 0.0), (1.0, INF), (64.0, 0.01))])
        for (a, aw), (b, bw) in zip(*res):
            same(b, a, f"synthetic, tile {tile} {keys}: colours")
            same(bw, aw, f"synthetic, tile {tile} {keys}: weight")
        m = res[1][-1][1] - cnt.astype(F)
        assert ((cnt == 0) & (m > 0)).any() and ((cnt == 0) & (m == 0)).any()


def test_default_variant_on_frames_rendered_on_the_gpu(gpu):
    """No environment override; history and frame rendered by the GPU's own path kernels and captured
    on the GPU, a window of feature buffers asked for first (so the planes have to grow), two
    captures in a chain: equal to the numpy statement applied twice."""
    name, W, H = "cornell", 65, 49
    cam0, sp = scene(name, W, H)
    cam1, cam2 = moved(cam0, ("a",), W, H), moved(moved(cam0, ("a",), W, H), ("left",), W, H)
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
        r.history_capture()
        r.reset_accum()
        r.set_camera(cam2)
        r.path_passes(*sched.next(1))
        colC, cntC = r.read_radiance()
        got, gw = r.reproject(weight=True)
    aov0, aov1, aov2 = (first_hit(sp, W, H, c, gpu) for c in (cam0, cam1, cam2))
    o1, w1, _ = np_reproject(colB, cntB, aov1, sp["refl"], hist_dict(cam0, colA, cntA.astype(F), aov0))
    o2, w2, _ = np_reproject(colC, cntC, aov2, sp["refl"], hist_dict(cam1, o1, w1, aov1))
    same(got, o2, "chain on the GPU vs numpy: colours")
    same(gw, w2, "chain on the GPU vs numpy: weight")
    assert (w2 > 5).any() and (w2 == 1).any()


def test_rgba_is_the_thresholds_applied_to_the_colours(gpu):
    name, W, H = "cornell", 65, 49
    cam0, sp, hc, hm, _ = history_of(name, W, H)
    cam1, col, cnt, _ = case_of(name, W, H, ("left",))
    with g.Renderer(sp, W, H, cam1, device=gpu) as r:
        r.write_radiance(col, cnt)
        r.history_write(cam0, hc, hm)
        out, w, px = r.reproject(weight=True, pixels=True)
        same(out, r.reproject(), "with and without pixels")
        assert np.array_equal(px, to_rgba(out)) and not np.array_equal(px, to_rgba(col))
        # pixels alone and weight alone through the C ABI
        only_px, only_w = np.empty((H, W, 4), np.uint8), np.empty((H, W), F)
        prm = g._lib.ReprojectParams(0, 64.0, 0.01)
        assert g.lib.bdpt_reproject(r._h, ctypes.byref(prm), None, None, ctypes.c_void_p(only_px.ctypes.data)) == 0
        assert g.lib.bdpt_reproject(r._h, ctypes.byref(prm), None, ctypes.c_void_p(only_w.ctypes.data), None) == 0
        assert np.array_equal(only_px, px)
        same(only_w, w, "weight alone")
        assert np.array_equal(r.read_pixels(), to_rgba(col))             # the context's own pixels: untouched


def test_scene_change_makes_the_history_absent(gpu):
    name, W, H = "cornell", 65, 49
    cam0, sp, hc, hm, _ = history_of(name, W, H)
    cam1, col, cnt, _ = case_of(name, W, H, ("a",))
    with g.Renderer(sp, W, H, cam1, device=gpu) as r:
        r.write_radiance(col, cnt)
        r.history_write(cam0, hc, hm)
        assert r.history_info()[0] is True and (r.reproject(weight=True)[1] != cnt.astype(F)).any()
        sp2 = sp.copy()
        assert g.sphere_key(sp2, 2, "4")
        r.set_scene(sp2)
        present, c0 = r.history_info()
        assert present is False and bytes(c0) == bytes(cam0)
        out, w = r.reproject(weight=True)
        same(out, col, "scene changed: out == colors")
        same(w, cnt.astype(F), "scene changed: weight == counter")
        r.history_clear()
        assert r.history_info()[0] is False


@pytest.mark.parametrize("streams", [0, 1])
def test_passes_after_capture_and_reproject_equal_passes_without_them(gpu, streams):
    assert_non_interference(gpu, "cornell_glass", 65, 49, streams=streams)


def test_errors(gpu):
    assert_errors(gpu)
    cam, sp = scene("cornell", 20, 19)
    with g.Renderer(sp, 20, 19, cam, devices=[gpu, gpu]) as r:          # a multi-device context
        col, w = np.zeros((19, 20, 3), F), np.ones((19, 20), F)
        for call in (r.reproject, r.history_capture, r.history_clear, r.history_read,
                     lambda: r.history_write(cam, col, w)):
            with pytest.raises(g.BdptError) as e:
                call()
            assert e.value.code == g._lib.BDPT_EINVAL
        assert g.lib.bdpt_history_info(r._h, None, None) == g._lib.BDPT_EINVAL
