"""First-hit feature buffers on the GPU (bdpt_aov_kernel, csrc/bdpt_kernels.hip, launched by
csrc/bdpt_frame.cpp): against the reference-written fixtures tests/golden/ref_aov_*.npz (the
reference's colours of an all-emitter
scene are e[id] * fabs(dp), tests/golden/make_ref_aov_golden.py), against the CPU backend on all six
planes, against the path kernel of the same context, over windows, and for side effects.  Every
comparison is on the float bits; no tolerance anywhere.  Sizes are not multiples of the kernel's
8x8 / 64x1 wave tiles or 32x8 / 64x4 workgroup tiles, so every launch has partial tiles and more
than one workgroup where the frame is 65x49 or 40x33."""
import numpy as np
import pytest

import gpu_bidirectional_raytracer_amd as g
from aov_common import (CASES, CLOCKS, assert_errors, assert_matches_reference, assert_non_interference,
                        assert_only_own_clock_answers, assert_window_slices, load_case, probe_colors,
                        render_fixture, same, same_aov, scene)

pytestmark = pytest.mark.gpu

CPU = -1
SID = 7
# (scene, W, H, traversal): cornell_glass by the brute scan, complex (783 spheres) on the tree
SCENES_VS_CPU = [("cornell_glass", 65, 49, None), ("complex", 40, 33, "bvh")]


@pytest.fixture(scope="module")
def cpu_planes():
    """The CPU backend's planes of SCENES_VS_CPU, jittered (table seed 15, sid 7) and not: computed
    once, read by several tests, never modified."""
    out = {}
    for name, W, H, _ in SCENES_VS_CPU:
        cam, sp = scene(name, W, H)
        with g.Renderer(sp, W, H, cam, device=CPU) as r:
            r.generate_rand(15)
            out[name] = {True: r.render_aov(sid=SID), False: r.render_aov()}
    return out


@pytest.mark.parametrize("name", CASES)
def test_fixture_colours_are_e_times_abs_dp(gpu, name):
    fx = load_case(name)
    aov, trav = render_fixture(fx, gpu)
    assert_matches_reference(fx, aov, name)
    assert trav == ("bvh" if name == "complex" else "brute")          # auto: the tree when the scene has one


@pytest.mark.parametrize("traversal", ["brute", "bvh"])
def test_complex_fixture_by_brute_scan_and_by_bvh(gpu, traversal):
    fx = load_case("complex")
    aov, trav = render_fixture(fx, gpu, traversal)
    assert trav == traversal                                           # the tree was (not) walked
    assert_matches_reference(fx, aov, f"complex {traversal}")


@pytest.mark.parametrize("jitter", [True, False])
@pytest.mark.parametrize("name,W,H,traversal", SCENES_VS_CPU)
def test_gpu_equals_cpu_backend_on_all_planes(gpu, cpu_planes, name, W, H, traversal, jitter):
    cam, sp = scene(name, W, H)
    with g.Renderer(sp, W, H, cam, device=gpu) as r:
        if traversal:
            r.set_traversal(traversal)
        if jitter:
            r.generate_rand(15)
        aov = r.render_aov(sid=SID if jitter else None)
        assert r.last_aov_traversal == (traversal or "brute")
        same_aov(aov, cpu_planes[name][jitter], f"{name} {W}x{H} jitter={jitter}")
        if name == "complex":                                          # and the other traversal agrees
            r.set_traversal("brute")
            same_aov(r.render_aov(sid=SID if jitter else None), aov, "complex brute vs bvh")
            assert r.last_aov_traversal == "brute"
    assert (aov["id"] >= 0).any()


@pytest.mark.parametrize("name", ["cornell_glass", "complex"])
def test_path_kernel_of_the_same_context_agrees(gpu, name):
    """Self-probe on the GPU alone: one path pass over the all-emitter scene returns e[id] * |dp|
    (device.cu:651-660) -- the path kernel's own first hit -- and render_aov gives the same."""
    W, H = 65, 49
    cam, sp = scene(name, W, H, probe=True)
    with g.Renderer(sp, W, H, cam, device=gpu) as r:
        r.light_pass(3)                                                # table seed 15
        aov = r.render_aov(sid=SID)
        r.path_passes([SID], [1])
        col, cnt = r.read_radiance()
        assert r.last_traversal == r.last_aov_traversal
    assert (cnt == 1).all()
    same(probe_colors(sp, aov), col, f"{name}: e[id] * |dp| vs the path kernel's radiance")
    assert (aov["id"] >= 0).sum() > 100


@pytest.mark.parametrize("name,W,H,traversal", SCENES_VS_CPU)
def test_windows_and_pick_equal_slices(gpu, cpu_planes, name, W, H, traversal):
    """Windows off and on the tile boundaries, single rows and columns, the frame's corners."""
    cam, sp = scene(name, W, H)
    with g.Renderer(sp, W, H, cam, device=gpu) as r:
        if traversal:
            r.set_traversal(traversal)
        r.generate_rand(15)
        windows = [(7, 5, 9, 11), (32, 8, W - 32, 9), (1, 0, W - 1, 1), (W - 1, 0, 1, H), (8, 8, 16, 16),
                   (3, 4, 1, 1), (W - 1, H - 1, 1, 1), (0, 0, 1, 1)]
        assert_window_slices(r, cpu_planes[name][True], SID, windows, name)
        assert_window_slices(r, cpu_planes[name][False], None, windows[:1] + windows[-3:], name)
        same_aov(r.render_aov(sid=SID), cpu_planes[name][True], "the whole frame after the windows")


@pytest.mark.parametrize("streams", [0, 1])
def test_passes_after_render_aov_equal_passes_without_it(gpu, streams):
    assert_non_interference(gpu, "cornell_glass", 65, 49, streams=streams)


def test_errors(gpu):
    assert_errors(gpu)


@pytest.mark.parametrize("service", CLOCKS)
def test_only_the_service_that_ran_has_a_last_ms(gpu, service):
    """The five bdpt_last_*_ms readers share one clock scaffold (csrc/bdpt_frame.cpp): one service's
    call must not make another's reader answer, and the one that ran measured a device interval."""
    assert_only_own_clock_answers(gpu, service)
