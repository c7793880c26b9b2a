"""The out-of-range scenes (tests/range_scenes.py) without a GPU.  Each scene means what its name
says, by the oracle's range counters (oracle.RANGE_NAMES: how often a squared length outside
[2^-96, 2^126) reaches a normalisation, how many NEE terms lie outside [2^-60, 2^60], ...) and by the
denormal and maximum colour values of its frame; every oracle frame is finite, which the GPU tests
need to compare on bits (x86 and gfx950 give generated NaNs different signs); the oracle equals the
reference's own code and the CPU backend equals the oracle, bit for bit; the black-surface exit
proof (csrc/bdpt_util.c bdpt_zero_exit_safe) holds where tests/test_gpu_range.py expects the
`zero_exit` feature; the host BVH builder makes a tree of the scaled tree scenes and its traversal
agrees with the every-sphere loops; and the previews of the CPU backend are NaN-free on the two
frames whose radiance is far out of range.

Frames 45x31, 6 passes of PassScheduler, table seed 0.  The floors are about a quarter of the counts
measured when the scenes were made (DESIGN.md section 2 has the table); a scene that misses a floor
is the wrong scene."""
import json
import os
import subprocess

import numpy as np
import pytest

import adversarial_scenes as A
import gpu_bidirectional_raytracer_amd as g
import oracle
import range_scenes as RS
from oracle import ref as R
from test_adversarial_cpu import bvh_check_exe, zero_exit  # noqa: F401  (a fixture and a helper)

CPU = -1
W, H = 45, 31
NPASS = 6
TINY = np.float32(2.0 ** -126)
NORM_SITES = ("norm_camera", "norm_normal", "norm_refr", "norm_nee", "norm_vlp", "norm_tangent")


@pytest.fixture(autouse=True)
def threads(monkeypatch):
    monkeypatch.setenv("BDPT_CPU_THREADS", "4")


@pytest.fixture(scope="module")
def rnd0():
    t = oracle.mt607(0)
    t.setflags(write=False)
    return t


def schedule(n=NPASS):
    s = g.PassScheduler()
    s.light()
    return s.next(n)


def make(name):
    cam, sp = RS.scene(name)
    g.update_camera(cam, W, H)
    return cam, sp


def denormal(a):
    return (a != 0) & (np.abs(a) < TINY)


@pytest.fixture(scope="module")
def frames(rnd0):
    """name -> dict(lp, light (range counters of the light pass), col, cnt, px, path (range counters
    of the path passes)) of the oracle, computed on first use."""
    cache = {}

    def get(name):
        if name not in cache:
            cam, sp = make(name)
            sid, vlp = schedule()
            lp, light = oracle.light_pass(sp, rnd0, 0, ranges=True)
            col, cnt, px, path = oracle.path_passes(sp, rnd0, cam, W, H, lp, sid, vlp, ranges=True)
            cache[name] = dict(lp=lp, light=light, col=col, cnt=cnt, px=px, path=path)
        return cache[name]
    return get


# ---- the scenes mean what their names say ------------------------------------------------------

def test_scaling_is_exact():
    cam0, sp0 = RS.scene("base")
    for name, k in RS.SCALES.items():
        cam, sp = RS.scene(name)
        ref_cam, ref = (cam0, sp0) if name not in RS.TREES else A.big_brute(200)
        s = 2.0 ** k
        assert np.array_equal(sp["rad"].astype(np.float64), ref["rad"].astype(np.float64) * s), name
        assert np.array_equal(sp["p"].astype(np.float64), ref["p"].astype(np.float64) * s), name
        assert (cam.orig.z, cam.target.y) == (ref_cam.orig.z * s, ref_cam.target.y * s)
        for f in ("e", "c", "refl"):
            assert np.array_equal(sp[f], ref[f])
    assert all(len(RS.scene(n)[1]) <= 16 for n in RS.SMALL)         # the specialised kernels unroll them


def test_counters_do_not_change_the_frame(rnd0):
    """The counting calls return the floats of the plain calls."""
    cam, sp = make("pin_light")
    sid, vlp = schedule()
    lp = oracle.light_pass(sp, rnd0, 0)
    lp2, light = oracle.light_pass(sp, rnd0, 0, ranges=True)
    assert lp.tobytes() == lp2.tobytes() and set(light) == set(oracle.RANGE_NAMES)
    plain = oracle.path_passes(sp, rnd0, cam, W, H, lp, sid, vlp)
    *counted, stats, path = oracle.path_passes(sp, rnd0, cam, W, H, lp, sid, vlp, stats=True, ranges=True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(plain, counted))
    assert set(path) == set(oracle.RANGE_NAMES) and stats["samples"] == W * H * NPASS
    assert path["nee_in"] + path["nee_out"] <= stats["diffuse"]      # at most one emitter's term per vertex
    assert sum(light.values()) > 0 and light["nee_in"] == light["nee_out"] == 0


def test_base_is_in_range(frames):
    for name in ("base", "near", "bright", "dim", "dimmer"):
        f = frames(name)
        assert f["path"]["nee_in"] >= 5000 and f["path"]["nee_out"] == 0, (name, f["path"])
        assert all(f["path"][k] == 0 for k in NORM_SITES + ("cam_w_out",)), (name, f["path"])
        assert f["light"]["norm_light"] == 0


@pytest.mark.parametrize("name", ["far", "vast", "big_far", "big_vast"])
def test_scaled_scenes_take_the_library_division(frames, name):
    path = frames(name)["path"]
    print(name, path, frames(name)["light"])
    assert path["nee_out"] >= 1000 and path["nee_in"] == 0, path


@pytest.mark.parametrize("name", ["vast", "big_vast"])
def test_vast_normalises_out_of_range(frames, name):
    f = frames(name)
    assert sum(f["path"][k] for k in NORM_SITES) >= 10000, f["path"]
    assert f["path"]["norm_camera"] == W * H * NPASS and f["path"]["norm_normal"] >= 10000
    assert f["light"]["norm_light"] >= 1000
    far = frames("far" if name == "vast" else "big_far")
    assert all(far["path"][k] == 0 for k in NORM_SITES) and far["light"]["norm_light"] == 0


def test_pin_light_is_on_both_sides(frames):
    f = frames("pin_light")
    print(f["path"], f["light"])
    assert f["path"]["nee_in"] >= 1000 and f["path"]["nee_out"] >= 1000
    assert f["light"]["norm_light"] >= 1000


def test_emission_scenes_reach_the_ends_of_float32(frames):
    dim, dimmer, bright = (frames(n) for n in ("dim", "dimmer", "bright"))
    n = dim["col"].size
    print("denormal colour values: dim", int(denormal(dim["col"]).sum()), "dimmer", int(denormal(dimmer["col"]).sum()),
          "of", n, "; denormal VLP radiance values (dimmer):", int(denormal(dimmer["lp"]["rad"]).sum()),
          "; bright max", float(bright["col"].max()))
    assert denormal(dim["col"]).sum() >= 0.01 * n
    assert denormal(dimmer["col"]).sum() >= 0.90 * n
    assert denormal(dimmer["lp"]["rad"]).sum() >= 1000
    assert bright["col"].max() >= 1e35


def id_plane(cam, sp):
    g.update_camera(cam, W, H)
    with g.Renderer(sp, W, H, cam, device=CPU) as r:
        aov = r.render_aov(planes=("id", "t"))
    return aov["id"], aov["t"]


def test_horizon_is_on_both_sides_of_the_rule(frames):
    """NEAR is shown (finite distances far above every other scene's), DOME's distance is +inf and
    it is shown nowhere; scaled by 1/2 DOME's rad^2 is finite and it fills what NEAR leaves."""
    cam, sp = RS.scene("horizon")
    with np.errstate(over="ignore"):
        assert np.float32(sp["rad"][RS.H_DOME]) * np.float32(sp["rad"][RS.H_DOME]) == np.inf
    ids, t = id_plane(cam, sp)
    near = ids == RS.H_NEAR
    assert near.sum() >= 20 and (ids == RS.H_DOME).sum() == 0 and (ids[~near] == -1).all()
    assert np.isfinite(t[near]).all() and t[near].min() > 1e18 and t[near].max() < 1e20
    cam, sp = RS.horizon(-1)
    assert np.isfinite(np.float32(sp["rad"][RS.H_DOME]) * np.float32(sp["rad"][RS.H_DOME]))
    ids2, t2 = id_plane(cam, sp)
    assert np.array_equal(ids2 == RS.H_NEAR, near) and (ids2[~near] == RS.H_DOME).all() and (~near).sum() >= 20
    assert t2[~near].max() < 1e20
    f = frames("horizon")
    assert f["path"]["norm_normal"] >= 1000                       # NEAR's normals: squared length >= 2^126


@pytest.mark.parametrize("name", RS.NAMES)
def test_oracle_frame_is_finite(frames, name):
    f = frames(name)
    assert np.isfinite(f["col"]).all(), f"{name}: colours"
    for k in ("hp", "rad", "nl"):
        assert np.isfinite(f["lp"][k]).all(), f"{name}: light paths' {k}"
    assert (f["cnt"] == NPASS).all()
    if name != "horizon":
        assert (f["col"] != 0).mean() >= 0.90, (name, float((f["col"] != 0).mean()))


def test_no_sweep_scene_reaches_the_tiny_dets(frames):
    """det in (0, 2^-96) and negative denormal det: no scene gets there (they are function-level
    cases); if one ever does, its name should say so."""
    for name in RS.NAMES:
        f = frames(name)
        assert f["path"]["det_tiny"] == f["path"]["det_neg_denormal"] == 0, name
        assert f["path"]["second_root"] > 0


# ---- the black-surface exit proof ----------------------------------------------------------------

def test_black_surface_exit_proof_on_the_range_scenes():
    for name in RS.SMALL:
        assert zero_exit(RS.scene(name)[1]) == (name in RS.ZERO_EXIT), name
    # near: the emitter's gap to the ceiling, 4 in base, is 1/8 here, below the proof's absolute
    # floor of 1 (len >= ~1 bounds the NEE term); the scaled-up scenes keep it by 1e-4 * scale
    assert "near" not in RS.ZERO_EXIT and zero_exit(RS.scene("far")[1]) == zero_exit(RS.scene("vast")[1]) == 1
    assert zero_exit(RS.scene("pin_light")[1]) == 0                  # radius below 2^-16 of the scale
    assert zero_exit(RS.scene("bright", emission=3e37)[1]) == 0      # the bound: 1.1 * e * 4 pi r^2 >= 1e38
    assert zero_exit(RS.scene("bright", emission=RS.PREVIEW_BRIGHT_E)[1]) == 1
    for name in RS.TREES:
        assert zero_exit(RS.scene(name)[1]) == 1


# ---- three ways to the same frame ----------------------------------------------------------------

@pytest.mark.skipif(not R.available(), reason="no reference build and no reference tree")
@pytest.mark.parametrize("name", RS.NAMES)
def test_oracle_equals_reference(rnd0, name):
    from test_ref_parity import assert_frame_equal, both
    cam, sp = make(name)
    sid, vlp = schedule()
    o, r = both(R.ref(), sp, rnd0, oracle.camera_array(cam), W, H, sid, vlp)
    assert_frame_equal(o, r, name)
    assert (r[2] == len(sid)).all()


@pytest.mark.parametrize("name", RS.NAMES)
def test_cpu_backend_equals_oracle(frames, name):
    cam, sp = make(name)
    sid, vlp = schedule()
    with g.Renderer(sp, W, H, cam, device=CPU) as r:
        r.light_pass(0)
        r.path_passes(sid, vlp)
        col, cnt = r.read_radiance()
        px = r.read_pixels()
        lp = r.read_lightpaths()
    f = frames(name)
    assert lp.tobytes() == f["lp"].tobytes(), f"{name}: light paths differ"
    assert np.array_equal(cnt, f["cnt"])
    bad = int((col.view(np.uint32) != f["col"].view(np.uint32)).sum())
    assert bad == 0, f"{name}: {bad} colour values differ"
    assert np.array_equal(px, f["px"])


# ---- the host BVH ----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", RS.TREES)
def test_host_bvh_builds_a_tree_and_traverses(bvh_check_exe, tmp_path, name):  # noqa: F811
    cam, sp = RS.scene(name)
    path = str(tmp_path / (name + ".scn"))
    A.write_scn(path, cam, sp)
    cam2, sp2 = g.read_scene(path)
    assert sp2.tobytes() == sp.tobytes() and (cam2.orig.z, cam2.target.y) == (cam.orig.z, cam.target.y)
    out = subprocess.run([bvh_check_exe, path, "100000", "5"], capture_output=True, text=True)
    rec = json.loads(out.stdout)
    print(name, rec)
    assert out.returncode == 0 and rec["bvh"], (name, out.stdout, out.stderr)
    assert (rec["bvh_spheres"], rec["walls"]) == (194, 6), rec
    assert rec["bad_closest"] == 0 and rec["bad_shadow"] == 0 and rec["rays"] == 100000, rec
    assert rec["hits"] > 50000


# ---- the previews on out-of-range radiance ---------------------------------------------------------

@pytest.mark.parametrize("name", ["bright", "dimmer"])
def test_cpu_previews_are_nan_free(name):
    """The condition of test_gpu_range.py's preview cases: no NaN in any output of the CPU backend
    (+inf is allowed: squares of colour differences overflow by design)."""
    out = RS.preview_outputs(name, CPU)
    for key, a in out.items():
        assert not np.isnan(np.asarray(a, np.float64)).any(), f"{name}: NaN in {key}"
    assert len(out) >= 20 and np.isfinite(out["frame"]).all() and (out["counter"] == NPASS).all()
    assert out["noise_valid_pixels"] > 0 and (out["reproject_weight"] > 1).any()
    if name == "bright":
        assert out["frame"].max() >= 1e35
    else:
        assert denormal(out["frame"]).mean() >= 0.9
