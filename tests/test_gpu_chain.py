"""Chain buffers on the GPU (bdpt_chain_kernel, csrc/bdpt_kernels.hip, launched by
csrc/bdpt_frame.cpp): against the CPU backend and the numpy statement of the definition
(tests/chain_common.py) on all ten planes, against the reference-written fixtures
tests/golden/ref_chain_*.npz, against the path kernel of the same context, over windows, and for
side effects.  Every comparison is on the float bits; no tolerance anywhere.  Frames are 20x19 and
33x9: no multiples of the 8x8 / 64x1 wave tiles, more than one workgroup by rows (64x4) at 20x19."""
import numpy as np
import pytest

import gpu_bidirectional_raytracer_amd as g
from chain_common import (PLANES, assert_errors, assert_non_interference, camera_of, load_case, meta,
                          probe_chain_colors, render_case, same, same_chain, scene, set_table, statement_case)

pytestmark = pytest.mark.gpu

CPU = -1
CASES = [c["name"] for c in meta()["cases"]]


@pytest.fixture(scope="module")
def cpu_chains():
    """The CPU backend's planes of every fixture, its own spheres and the probe scene: computed
    once, read by several tests, never modified."""
    out = {}
    for name in CASES:
        fx = load_case(name)
        out[name] = (fx, render_case(fx, CPU, fx["spheres"]), render_case(fx, CPU, fx["scene_spheres"]))
    return out


@pytest.mark.parametrize("name", CASES)
def test_gpu_equals_cpu_backend_and_statement(gpu, cpu_chains, name):
    fx, cpu_probe, cpu_own = cpu_chains[name]
    probe, own = render_case(fx, gpu, fx["spheres"]), render_case(fx, gpu, fx["scene_spheres"])
    for branch in ("pass", "transmit"):
        same_chain(probe[branch], cpu_probe[branch], f"{name} probe {branch} vs the CPU backend")
        same_chain(own[branch], cpu_own[branch], f"{name} {branch} vs the CPU backend")
        same_chain(own[branch], statement_case(fx, fx["scene_spheres"], branch), f"{name} {branch} vs the statement")
    same(probe_chain_colors(fx["spheres"], probe["pass"]), fx["colors"], f"{name}: the reference's colours")


@pytest.mark.parametrize("traversal", ["brute", "bvh"])
def test_complex_by_brute_scan_and_by_bvh(gpu, cpu_chains, traversal):
    fx, cpu_probe, cpu_own = cpu_chains["complex_s15"]
    probe = render_case(fx, gpu, fx["spheres"], traversal)
    own = render_case(fx, gpu, fx["scene_spheres"], traversal)
    for branch in ("pass", "transmit"):
        same_chain(probe[branch], cpu_probe[branch], f"complex probe {traversal} {branch}")
        same_chain(own[branch], cpu_own[branch], f"complex {traversal} {branch}")
    same(probe_chain_colors(fx["spheres"], probe["pass"]), fx["colors"], f"complex {traversal}: the reference's colours")


@pytest.mark.parametrize("streams", [0, 1])
@pytest.mark.parametrize("name", ["mirror_s15", "glass_s15", "hall_s15", "complex_s15"])
def test_path_kernel_of_the_same_context_agrees(gpu, name, streams):
    """One path pass over the probe scene with a zero light-path table returns throughput *
    (|dp| * e[id]) of the pass's own chain (device.cu:651-660); render_chain gives the same."""
    fx = load_case(name)
    with g.Renderer(fx["spheres"], fx["W"], fx["H"], camera_of(fx), device=gpu) as r:
        r.set_streams(streams)
        set_table(r, fx)
        chain = r.render_chain(sid=fx["sid"], branch="pass")
        r.path_passes([fx["sid"]], [1])
        col, cnt = r.read_radiance()
    assert (cnt == 1).all()
    same(probe_chain_colors(fx["spheres"], chain), col, f"{name}: the path kernel's radiance")


def test_windows_equal_slices(gpu, cpu_chains):
    """A 1x1 and an odd window, jittered and not; the whole frame again afterwards."""
    fx, _, cpu_own = cpu_chains["mirror_s15"]
    with g.Renderer(fx["scene_spheres"], fx["W"], fx["H"], camera_of(fx), device=gpu) as r:
        set_table(r, fx)
        whole0 = r.render_chain()
        for x0, y0, w, h in [(7, 3, 13, 5), (3, 4, 1, 1), (19, 18, 1, 1), (0, 0, 20, 1)]:
            win = r.render_chain(sid=fx["sid"], branch="pass", window=(x0, y0, w, h))
            win0 = r.render_chain(window=(x0, y0, w, h))
            for k in PLANES:
                same(win[k], cpu_own["pass"][k][y0:y0 + h, x0:x0 + w], f"window {(x0, y0, w, h)} {k}")
                same(win0[k], whole0[k][y0:y0 + h, x0:x0 + w], f"unjittered window {(x0, y0, w, h)} {k}")
        same_chain(r.render_chain(sid=fx["sid"], branch="pass"), cpu_own["pass"], "the whole frame after the windows")
    with g.Renderer(fx["scene_spheres"], fx["W"], fx["H"], camera_of(fx), device=CPU) as r:
        same_chain(whole0, r.render_chain(), "unjittered vs the CPU backend")


@pytest.mark.parametrize("streams", [0, 1])
def test_queued_behind_unsynchronised_passes(gpu, streams):
    assert_non_interference(gpu, "cornell_mirror", 33, 9, streams=streams, queued=True)


def test_errors(gpu):
    assert_errors(gpu)
    cam, sp = scene("cornell_mirror", 20, 19)
    with g.Renderer(sp, 20, 19, cam, devices=[gpu, gpu]) as r:          # a multi-device context
        with pytest.raises(g.BdptError) as e:
            r.render_chain()
        assert e.value.code == g._lib.BDPT_EINVAL
