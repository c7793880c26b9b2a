"""The out-of-range scenes (tests/range_scenes.py) through the HIP kernels, bit for bit against the
oracle -- which tests/test_range_cpu.py holds to the reference's own code on the same scenes, and
whose range counters prove there that each scene reaches what its name says: the library division of
the NEE term (far, vast, pin_light), the sqrtf / 1.f/x fallback of the normalisations (vast,
pin_light's light pass, horizon), denormal radiance through the sparse fold, the running mean and the
units' atomics (dim, dimmer), radiance near the black-surface exit's bound (bright), the `d < 1e20`
rule on a distance of +inf (horizon), and the BVH set-up's margins at 2^31 and 2^50 (big_far,
big_vast).  Every other scene of the suite lives in coordinates 0..300 and emission 1..30, where none
of that code runs.

Every kernel mode of tests/accum_modes.py runs on every scene, specialised and not, and proves
afterwards that it ran.  The first-hit kernel and the previews (denoise, noise estimate, reproject,
preview_denoise) are compared with the CPU backend.  Frames 45x31, 6 passes of PassScheduler (8 where
the mode needs launches of 8), table seed 0.  No tolerance anywhere; the oracle's frames are finite
(asserted in the CPU test), so every comparison is on the bits."""
import dataclasses

import numpy as np
import pytest

import accum_modes as am
import gpu_bidirectional_raytracer_amd as g
import oracle
import range_scenes as RS
from aov_common import PLANES, bits, same

pytestmark = pytest.mark.gpu

CPU = -1
W, H = 45, 31
SID = 7
BRUTE_MODES = [m for m in am.MODES if not m.bvh]
# (mode, specialize): every mode as listed, and the specialised ones again with set_specialize(False),
# where pools and units have no kernel and the launch falls to the precompiled pass-stream instance
SMALL_CASES = [(m.name, m.specialize) for m in BRUTE_MODES] + [(m.name, False) for m in BRUTE_MODES if m.specialize]
TREE_MODES = ["bvh_fused", "bvh_one_per_lane", "precompiled_fused", "precompiled_one_per_lane"]
AOV_SCENES = ["far", "vast", "near", "horizon", "big_far", "big_vast"]
VARIANTS = [("64", "1"), ("64", "0"), ("8", "1"), ("8", "0")]     # BDPT_DENOISE_TILE, BDPT_DENOISE_LDS


def schedule(n):
    s = g.PassScheduler()
    s.light()
    return s.next(n)


def make(name, device):
    cam, sp = RS.scene(name)
    g.update_camera(cam, W, H)
    return g.Renderer(sp, W, H, cam, device=device), cam, sp


@pytest.fixture(scope="module")
def rnd0():
    t = oracle.mt607(0)
    t.setflags(write=False)
    return t


@pytest.fixture(scope="module")
def light_paths(rnd0):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = oracle.light_pass(RS.scene(name)[1], rnd0, 0)
            cache[name].setflags(write=False)
        return cache[name]
    return get


@pytest.fixture(scope="module")
def oracle_frames(rnd0, light_paths):
    """(colors, counter, pixels) of the oracle per (scene, passes), computed once and left unchanged."""
    cache = {}

    def get(name, npass):
        if (name, npass) not in cache:
            cam, sp = RS.scene(name)
            g.update_camera(cam, W, H)
            sid, vlp = schedule(npass)
            cache[name, npass] = oracle.path_passes(sp, rnd0, cam, W, H, light_paths(name), sid, vlp)
            assert np.isfinite(cache[name, npass][0]).all()
        return cache[name, npass]
    return get


def assert_frame(r, want, what):
    col, cnt = r.read_radiance()
    ocol, ocnt, opx = want
    assert np.array_equal(cnt, ocnt), f"{what}: counters differ"
    bad = np.argwhere(bits(col) != bits(ocol))
    assert len(bad) == 0, (f"{what}: {len(bad)} of {col.size} colour values differ, first at {bad[:4].tolist()}: "
                           f"{[float(col[tuple(b)]) for b in bad[:4]]} for {[float(ocol[tuple(b)]) for b in bad[:4]]}")
    assert np.array_equal(r.read_pixels(), opx), f"{what}: pixels differ"


# ---- the light pass ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", RS.NAMES)
def test_light_pass_equals_oracle(gpu, light_paths, name):
    r, cam, sp = make(name, gpu)
    with r:
        r.light_pass(0)
        lp = r.read_lightpaths()
    want = light_paths(name)
    diff = int((lp.view(np.uint32).reshape(len(lp), -1) != want.view(np.uint32).reshape(len(lp), -1)).any(axis=1).sum())
    assert diff == 0, f"{name}: {diff} of {len(lp)} light paths differ"


# ---- the path kernels ---------------------------------------------------------------------------

def run_mode(r, mode, name, oracle_frames, monkeypatch):
    npass = max(6, mode.min_launch)
    sid, vlp = schedule(npass)
    r.light_pass(0)
    am._call(r, mode, sid, vlp, None)
    return oracle_frames(name, npass)


@pytest.mark.parametrize("mode_name,specialize", SMALL_CASES)
@pytest.mark.parametrize("name", RS.SMALL)
def test_small_scene_every_mode_bit_exact(gpu, oracle_frames, monkeypatch, name, mode_name, specialize):
    mode = am.BY_NAME[mode_name]
    if not specialize:
        mode = dataclasses.replace(mode, specialize=False, feature=None)
    am.force_env(mode, None, monkeypatch)
    r, cam, sp = make(name, gpu)
    with r:
        r.set_specialize(specialize)
        want = run_mode(r, mode, name, oracle_frames, monkeypatch)
        assert r.last_traversal == "brute" and r.last_specialized == specialize, r.specialize_status
        feats = r.last_features
        assert ("specialized" in feats) == specialize
        assert ("zero_exit" in feats) == (specialize and name in RS.ZERO_EXIT), (name, feats)
        assert_frame(r, want, f"{name} {mode_name} specialize {specialize}")


@pytest.mark.parametrize("mode_name", TREE_MODES)
@pytest.mark.parametrize("name", RS.TREES)
def test_tree_scene_bit_exact(gpu, oracle_frames, monkeypatch, name, mode_name):
    mode = am.BY_NAME[mode_name]
    am.force_env(mode, None, monkeypatch)
    r, cam, sp = make(name, gpu)
    with r:
        assert r.has_bvh
        r.set_specialize(False)
        r.set_traversal("bvh" if mode.bvh else "brute")
        want = run_mode(r, mode, name, oracle_frames, monkeypatch)
        assert ("bvh" in r.last_features) == mode.bvh
        assert_frame(r, want, f"{name} {mode_name}")


# ---- the first hit ------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cpu_planes():
    """The CPU backend's planes per scene, jittered (table seed 15, sid 7) and not."""
    cache = {}

    def get(name):
        if name not in cache:
            r, cam, sp = make(name, CPU)
            with r:
                r.generate_rand(15)
                cache[name] = {True: r.render_aov(sid=SID), False: r.render_aov()}
        return cache[name]
    return get


@pytest.mark.parametrize("name", AOV_SCENES)
def test_first_hit_equals_cpu_backend(gpu, cpu_planes, name):
    want = cpu_planes(name)
    for k in PLANES:                                        # the condition of comparing on bits
        assert not np.isnan(want[True][k]).any() and not np.isnan(want[False][k]).any(), (name, k)
    ids = want[False]["id"]
    ys, xs = np.nonzero(ids >= 0)
    picks = sorted({(int(xs[k]), int(ys[k])) for k in np.linspace(0, len(xs) - 1, 12).astype(int)})
    miss = np.argwhere(ids < 0)[:2]
    r, cam, sp = make(name, gpu)
    with r:
        r.generate_rand(15)
        for traversal in (("brute", "bvh") if name in RS.TREES else ("brute",)):
            r.set_traversal(traversal)
            for jitter in (True, False):
                aov = r.render_aov(sid=SID if jitter else None)
                assert r.last_aov_traversal == traversal
                for k in PLANES:
                    same(aov[k], want[jitter][k], f"{name} {traversal} jitter={jitter}: {k}")
            for x, y in picks + [(int(x), int(y)) for y, x in miss]:
                i, t = r.pick(x, y)
                assert i == ids[y, x], f"{name} {traversal}: pick({x}, {y}) = {i}, the plane has {ids[y, x]}"
                assert np.float32(t).view(np.uint32) == bits(want[False]["t"])[y, x]
    if name == "horizon":
        assert (ids == RS.H_NEAR).sum() >= 20 and (ids == RS.H_DOME).sum() == 0 and (ids == -1).sum() >= 20
    else:
        assert (ids >= 0).all() and len(np.unique(ids)) >= 8


# ---- the previews on out-of-range radiance -------------------------------------------------------

@pytest.fixture(scope="module")
def cpu_previews():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = RS.preview_outputs(name, CPU)
        return cache[name]
    return get


@pytest.mark.parametrize("tile,lds", VARIANTS)
@pytest.mark.parametrize("name", ["bright", "dimmer"])
def test_previews_equal_cpu_backend(gpu, cpu_previews, monkeypatch, name, tile, lds):
    monkeypatch.setenv("BDPT_DENOISE_TILE", tile)
    monkeypatch.setenv("BDPT_DENOISE_LDS", lds)
    monkeypatch.setenv("BDPT_REPROJECT_TILE", tile)
    want = cpu_previews(name)
    got = RS.preview_outputs(name, gpu)
    assert list(got) == list(want)
    for k in want:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert not np.isnan(np.asarray(b, np.float64)).any(), f"{name}: the CPU backend's {k} has a NaN"
        assert a.dtype == b.dtype and a.shape == b.shape, (k, a.dtype, b.dtype)
        bad = int((a.view(np.uint8) != b.view(np.uint8)).reshape(a.size, -1).any(axis=1).sum()) if a.size else 0
        assert bad == 0, f"{name} tile {tile} lds {lds}: {bad} of {a.size} values of {k} differ"
