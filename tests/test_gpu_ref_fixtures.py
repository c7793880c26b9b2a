"""The HIP kernels against fixtures written by the reference's own code.

tests/golden/ref_*.npz come from oracle/_ref/libref.so -- the reference's device.cu and
MersenneTwister_kernel.cu compiled as host C++ (tests/golden/make_ref_golden.py; the CPU module
tests/test_ref_parity.py checks that regenerating reproduces them).  Here the product renders the
stored inputs through `Renderer` and must give the stored outputs bit for bit: the MT607 table of
seed 15 (generate_rand), the light pass (dev_lp: digest and every 16th row), and path_passes at
the edges the index formulas device.cu:173,273,562,619 have -- a light pass at current_sample 3,
sids that wrap the table inside the frame (RAND_N-1 among them), vlp 4095, a 1x1 frame, a running
mean through the 30000 cap, no emitter, three emitters -- plus the 20x19 frames (one column past
the 19x19 launch block) of cornell, cornell_glass and caustic.  Only committed fixtures are read:
neither the library nor the reference tree is needed.  No tolerance anywhere."""
import json
import os

import numpy as np
import pytest

import gpu_bidirectional_raytracer_amd as g
import oracle
from conftest import GOLDEN
from make_ref_golden import LP_STRIDE, load_case, lp_rows

pytestmark = pytest.mark.gpu

REF_META = json.load(open(os.path.join(GOLDEN, "ref_meta.json")))
CASES = [c["name"] for c in REF_META["cases"]]


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def run_renderer(case, device, streams=None):
    """A case (make_ref_golden.cases() entry or load_case() fixture) through one Renderer ->
    {lp, colors, counter, pixels}."""
    cam = g.Camera.from_buffer_copy(np.ascontiguousarray(case["camera"]).tobytes())
    with g.Renderer(case["spheres"], case["W"], case["H"], cam, device=device) as r:
        r.light_pass(case["current_sample"])
        if streams is not None:
            r.set_streams(streams)
        if case.get("colors0") is not None:
            r.write_radiance(case["colors0"], case["counter0"])
        r.path_passes(case["sid"], case["vlp"])
        col, cnt = r.read_radiance()
        return {"lp": r.read_lightpaths(), "colors": col, "counter": cnt, "pixels": r.read_pixels()}


def assert_matches_fixture(got, fx, what):
    rows = lp_rows(got["lp"])
    assert np.array_equal(u32(rows[::LP_STRIDE]), u32(fx["lp_rows"])), f"{what}: dev_lp rows differ"
    assert oracle.fnv1a64(rows) == int(fx["lp_fnv"]), f"{what}: dev_lp digest differs"
    assert np.array_equal(got["counter"], fx["counter"]), f"{what}: counters differ"
    bad = int((u32(got["colors"]) != u32(fx["colors"])).sum())
    assert bad == 0, f"{what}: {bad} of {fx['colors'].size} radiance values differ"
    assert np.array_equal(got["pixels"], fx["pixels"]), f"{what}: pixels differ"


def test_generate_rand_seed15_matches_reference_table(gpu):
    """generate_rand(15) (the seed of a light pass at current_sample 3) against RandomGPU
    (MersenneTwister_kernel.cu:63-110) as the reference build ran it."""
    fx = np.load(os.path.join(GOLDEN, "ref_mt607.npz"))
    cam, sp = g.read_scene(os.path.join(g.SCENE_DIR, "simple.scn"))
    with g.Renderer(sp, 4, 4, g.update_camera(cam, 4, 4), device=gpu) as r:
        r.generate_rand(int(fx["seed"]))
        rnd = r.read_rand()
    assert np.array_equal(u32(rnd[fx["idx"]]), u32(fx["values"]))
    assert oracle.fnv1a64(rnd) == int(fx["fnv"])


@pytest.mark.parametrize("streams", [0, 1])
@pytest.mark.parametrize("name", CASES)
def test_renderer_matches_reference_fixture(gpu, name, streams):
    fx = load_case(name)
    got = run_renderer(fx, gpu, streams=streams)
    assert_matches_fixture(got, fx, f"{name} streams={streams}")
