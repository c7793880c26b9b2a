"""Part-full shadow rounds of the scene-specialised path kernels (bdpt_kernels.hip pf_round,
BDPT_PF_UNROLL): the straight-line bodies, one per lane-group count and sphere list, against the
oracle and against the same kernels built with the lane-group loop (-DBDPT_PF_UNROLL=0).

Frames of 2 x 1, 3 x 2, 8 x 1, 8 x 2 and 8 x 4 pixels hold at most 2, 6, 8, 16 and 32 live lanes per
wave, so their shadow steps queue at most 4, 12, 16, 32 and 64 rays: every round of the first four
is part-full, and together they reach every group count (lg = 5 .. 1); 97 x 65 adds full waves with
a part-full second round and both packed frame edges.  Scenes: cornell (9 spheres, 8 non-emitters:
VLP-only rounds take the non-emitters' list), cornell_2luci (two emitters: two light steps per vertex, the
second of NEE rays only), caustic (3 spheres: lg reduced to 2) and synthetic64
(64 spheres: lg <= 2 exceeds the unroll bound and keeps the loop, lg >= 3 is unrolled).

16 passes in one call, in the ordered in-kernel fold (units), a fixed S = 3 pass stream and pixel
pools.  The pool build leaves the switch off by default, so it is also run with it on.  Every
comparison is on the bits: colours, counters and pixels against the oracle (computed once per
scene and frame) and against the flag-off build, and every run proves through last_features and
device_mode that the specialised kernel of the mode ran.

These four scenes fix the sphere count and the emitters' indices; the sweep over counts 1..64 and
emitter positions (every (lane-group count, list) body, masked tails, both widths of the emitter
mask) lives in tests/test_gpu_sphere_counts.py, over the scenes of tests/count_scenes.py."""
import numpy as np
import pytest

import accum_modes as am
import gpu_bidirectional_raytracer_amd as g

pytestmark = pytest.mark.gpu

FRAMES = [(2, 1), (3, 2), (8, 1), (8, 2), (8, 4), (97, 65)]
SCENES = ["cornell", "cornell_2luci", "caustic", "synthetic64"]
MODES = ["units3", "fixed_s3", "pool2"]
NPASS = 16
OFF, ON = "-DBDPT_PF_UNROLL=0", "-DBDPT_PF_UNROLL=1"


def _render(mode, sc, gpu, monkeypatch, flags):
    """[state after light_pass, state after the call] of `sc` in `mode`, kernels built with
    BDPT_JIT_FLAGS = flags (None: the defaults)."""
    am.force_env(mode, None, monkeypatch)
    if flags is None:
        monkeypatch.delenv("BDPT_JIT_FLAGS", raising=False)
    else:
        monkeypatch.setenv("BDPT_JIT_FLAGS", flags)
    cam, sp = am.load_scene(sc)
    sid, vlp = am.schedule(NPASS)
    out = []
    with g.Renderer(sp, sc.width, sc.height, cam, device=gpu) as r:
        r.set_specialize(True)
        r.set_traversal("brute")                       # synthetic64 has a BVH; the lists are the brute kernels'
        r.light_pass(0)

        def state():
            col, cnt = r.read_radiance()
            out.append((col, cnt, r.read_pixels()))

        state()
        am._call(r, mode, sid, vlp, None)              # asserts the mode, the launch count, specialised
        what = f"{mode.name} {sc.scene} {sc.width}x{sc.height} flags {flags}"
        assert "specialized" in r.last_features, f"{what}: {r.last_features}: {r.specialize_status!r}"
        dm = r.device_mode()
        assert "specialized" in dm["features"] and "pass_streams" in dm["features"], f"{what}: {dm}"
        if mode.feature:
            assert mode.feature in dm["features"], f"{what}: {dm}"
        state()
    return out


@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: f"{f[0]}x{f[1]}")
@pytest.mark.parametrize("scene", SCENES)
@pytest.mark.parametrize("name", MODES)
def test_partfull_rounds(gpu, name, scene, frame, monkeypatch):
    mode = am.BY_NAME[name]
    sc = am.Scenario(f"partfull{frame[0]}x{frame[1]}", scene, (("passes", NPASS),), width=frame[0], height=frame[1])
    what = f"{name} {scene} {frame[0]}x{frame[1]}"
    off = _render(mode, sc, gpu, monkeypatch, OFF)
    am.check(sc, off, f"{what} loop")
    for flags in (None, ON) if mode.pool else (None,):
        got = _render(mode, sc, gpu, monkeypatch, flags)
        am.check(sc, got, f"{what} {flags or 'default'}")
        for a, b, part in zip(got[1], off[1], ("colors", "counter", "pixels")):
            am.same(np.asarray(a), np.asarray(b), f"{what} {flags or 'default'} vs {OFF}: {part}")
