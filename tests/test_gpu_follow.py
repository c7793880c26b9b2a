"""The sphere-following history on the GPU (bdpt_reproject_kernel with the table of offsets,
csrc/bdpt_frame_kernels.h; include/bdpt.h bdpt_history_follow) against the CPU backend
-- which tests/test_follow_cpu.py holds to the numpy statement -- and against that statement
directly.  Every comparison is on the float bits; no tolerance anywhere.  The frames have at most
65x49 pixels and none is a multiple of the 8x8 / 64x1 wave tiles or the 32x8 / 64x4 workgroup
tiles; both wave tiles are run, whichever of them is the default.  The CPU-side inputs and results
are computed once per module."""
import numpy as np
import pytest

import gpu_bidirectional_raytracer_amd as g
from aov_common import same, scene, schedule
from follow_common import (CASES, MOVED, SAME, assert_equal_results, assert_not_vacuous, case_id, inputs_of,
                           moved_spheres, np_follow, offsets, renderer, results, setup, statement, want)
from reproject_common import CPU, DEFAULTS, F, hist_dict

pytestmark = pytest.mark.gpu

TILES = ["64", "8"]                                      # BDPT_REPROJECT_TILE


@pytest.fixture(scope="module")
def cpu_results():
    """Per case: (the CPU backend's results, the statement's), read by both tile variants, never
    modified."""
    return {case: (results(CPU, case), want(case)) for case in CASES}


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_gpu_equals_cpu_backend_and_the_statement(gpu, cpu_results, monkeypatch, case, tile):
    monkeypatch.setenv("BDPT_REPROJECT_TILE", tile)
    assert_not_vacuous(case)
    got = results(gpu, case)
    cpu, stated = cpu_results[case]
    assert_equal_results(got, cpu, case, f"GPU (tile {tile}) vs the CPU backend")
    assert_equal_results(got, stated, case, f"GPU (tile {tile}) vs the statement")


@pytest.mark.parametrize("tile", TILES)
def test_follow_on_without_a_move_equals_follow_off(gpu, monkeypatch, tile):
    monkeypatch.setenv("BDPT_REPROJECT_TILE", tile)
    for case in (CASES[0], CASES[4], CASES[7]):
        i = inputs_of(case)
        res = []
        for on in (False, True):
            with renderer(gpu, case) as r:
                r.history_follow(on)
                r.history_write(i["cam0"], i["hc"], i["hm"])
                r.write_radiance(i["col"], i["cnt"])
                assert r.history_motion()[0] == SAME and r.history_info()[0] is True
                res.append([r.reproject(weight=True), r.reproject(weight=True, materials="all", plane_tol=0.0),
                            r.preview_denoise(weight=True)])
                r.history_capture()
                res[-1].append(r.history_read())
        for (a, aw), (b, bw) in zip(*res):
            same(b, a, f"{case_id(case)}: follow on, nothing moved: colours")
            same(bw, aw, f"{case_id(case)}: follow on, nothing moved: weight")
        assert (res[0][0][1] != i["cnt"].astype(F)).any()


def test_follow_off_a_moved_sphere_leaves_the_history_absent(gpu):
    case = CASES[0]
    i = inputs_of(case)
    with renderer(gpu, case) as r:
        setup(r, case)
        state, delta = r.history_motion()
        assert state == MOVED and r.history_info()[0] is False
        same(delta, i["delta"], "delta with follow off")
        out, w = r.reproject(weight=True)
        same(out, i["col"], "follow off: out == colors")
        same(w, i["cnt"].astype(F), "follow off: weight == counter")


@pytest.mark.parametrize("tile", TILES)
def test_a_second_move_after_a_capture_and_a_move_back(gpu, monkeypatch, tile):
    """S0 history, move sphere 6, capture, move sphere 7 (a new table), reproject == the statement
    applied twice; then the spheres back where the capture saw them (state 1: no table), and moved
    once more by the same step (the table the device already holds)."""
    monkeypatch.setenv("BDPT_REPROJECT_TILE", tile)
    case = CASES[0]
    name, W, H = case[:3]
    i = inputs_of(case)
    S2 = moved_spheres(i["S1"], ((7, "9"),))
    sid, vlp = schedule(1)
    with g.Renderer(S2, W, H, i["cam1"], device=CPU) as r:
        r.light_pass(0)
        r.path_passes(sid, vlp)
        col2, cnt2 = r.read_radiance()
        aov2 = r.render_aov()
    o1, w1, _ = statement(case, DEFAULTS)
    hist1 = hist_dict(i["cam1"], o1, w1, i["aov1"])
    o2, w2, _ = np_follow(col2, cnt2, aov2, S2["refl"], hist1, offsets(i["S1"], S2))
    o3, w3, _ = np_follow(i["col"], i["cnt"], i["aov1"], i["S1"]["refl"], hist1, np.zeros_like(i["delta"]))
    with renderer(gpu, case) as r:
        r.history_follow(True)
        setup(r, case)
        r.history_capture()
        assert r.history_motion()[0] == SAME
        r.set_scene(S2)
        r.write_radiance(col2, cnt2)
        for k in range(2):                                     # the second call finds the table in place
            got, gw = r.reproject(weight=True)
            same(got, o2, f"chain, call {k}: out")
            same(gw, w2, f"chain, call {k}: weight")
        r.set_scene(i["S1"])
        r.write_radiance(i["col"], i["cnt"])
        assert r.history_motion()[0] == SAME
        got, gw = r.reproject(weight=True)
        same(got, o3, "back where the capture saw them: out")
        same(gw, w3, "back where the capture saw them: weight")
        r.set_scene(S2)
        r.write_radiance(col2, cnt2)
        got, gw = r.reproject(weight=True)
        same(got, o2, "moved again by the same step: out")
        same(gw, w2, "moved again by the same step: weight")
    assert (w2 > 5).any()


def test_a_reprojection_queued_behind_unsynchronised_passes(gpu):
    """History captured under S0 on the GPU, sphere 6 moved, passes queued without a sync, then the
    reprojection at once: it saw the finished frame and equals the statement on it."""
    case = CASES[0]
    name, W, H = case[:3]
    i = inputs_of(case)
    sid, vlp = schedule(5)
    with g.Renderer(i["S0"], W, H, i["cam1"], device=gpu) as r:
        r.history_follow(True)
        r.light_pass(0)
        r.path_passes(sid[:4], vlp[:4])
        hc, cnt0 = r.read_radiance()
        aov0 = r.render_aov()
        r.history_capture()
        r.reset_accum()
        r.set_scene(i["S1"])
        r.light_pass(0)
        r.path_passes(sid[4:], vlp[4:], sync=False)
        got, gw = r.reproject(weight=True)
        col, cnt = r.read_radiance()
        aov1 = r.render_aov()
        assert r.last_reproject_ms() > 0.0
    assert (cnt == 1).all()
    o, w, taps = np_follow(col, cnt, aov1, i["S1"]["refl"], hist_dict(i["cam1"], hc, cnt0.astype(F), aov0), i["delta"])
    same(got, o, "queued behind unsynchronised passes: out")
    same(gw, w, "queued behind unsynchronised passes: weight")
    assert (taps[aov1["id"] == 6] > 0).any()


def test_errors(gpu):
    EINVAL = g._lib.BDPT_EINVAL
    cam, sp = scene("cornell_diff", 20, 19)
    with g.Renderer(sp, 20, 19, cam, devices=[gpu, gpu]) as r:          # a multi-device context
        for call in (r.history_follow, r.history_motion):
            with pytest.raises(g.BdptError) as e:
                call()
            assert e.value.code == EINVAL
    with g.Renderer(sp, 20, 19, cam, device=gpu) as r:
        delta = np.zeros((len(sp), 3), F)
        assert g.lib.bdpt_history_motion(r._h, None, delta.ctypes.data, len(sp) + 1) == EINVAL
        r.history_follow(True)
        with pytest.raises(g.BdptError) as e:                           # BDPT_DENOISE_THROUGH stays refused
            r.reproject(materials="through")
        assert e.value.code == EINVAL
