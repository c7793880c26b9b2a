"""First-hit feature buffers (include/bdpt.h bdpt_render_aov, bdpt_pick) on the CPU backend
(device = BDPT_DEVICE_CPU, csrc/bdpt_cpu.cpp bdpt_cpu_render_aov); runs without a GPU.

The reference has no feature buffers, but its path kernel returns e[id] * fabs(dp) for a scene of
emitters (device.cu:651-660): tests/golden/ref_aov_*.npz hold those colours as the reference's own
code wrote them (tests/golden/make_ref_aov_golden.py), and render_aov must reproduce them bit for
bit.  The other planes are tied to id and dp by identities evaluated in numpy float32 in the
reference's operation order.  No tolerance anywhere, except |dir| (2 ulp of 1, reasoned below)."""
import os

import numpy as np
import pytest

import gpu_bidirectional_raytracer_amd as g
import make_ref_aov_golden as mra
from aov_common import (AOV_META, CASES, PLANES, assert_errors, assert_matches_reference, assert_non_interference,
                        assert_window_slices, bits, load_case, render_fixture, same)
from conftest import GOLDEN, SCENES
from oracle import ref as R

CPU = -1


@pytest.fixture(autouse=True)
def threads(monkeypatch):
    monkeypatch.setenv("BDPT_CPU_THREADS", "4")


@pytest.fixture(scope="module")
def rendered():
    """Every fixture through the CPU backend, once."""
    os.environ.setdefault("BDPT_CPU_THREADS", "4")
    return {name: (load_case(name), render_fixture(load_case(name), CPU)[0]) for name in CASES}


@pytest.mark.parametrize("name", CASES)
def test_fixture_colours_are_e_times_abs_dp(rendered, name):
    fx, aov = rendered[name]
    assert_matches_reference(fx, aov, name)


def test_fixtures_cover_what_they_claim(rendered):
    """Misses exist in caustic and complex, complex shows 30 of its 783 spheres, the wrap case wraps
    inside the frame, and the meta file describes the committed files."""
    assert CASES == [c["name"] for c in mra.cases()]
    for m in AOV_META["cases"]:
        fx, aov = rendered[m["name"]]
        assert m["size"] == [fx["W"], fx["H"]] and m["sid"] == fx["sid"] and m["table_seed"] == fx["table_seed"]
        assert m["hit_pixels"] == int((aov["id"] >= 0).sum()) and m["spheres"] == len(fx["spheres"])
        assert os.path.getsize(os.path.join(GOLDEN, f"ref_aov_{m['name']}.npz")) <= 32768
        ids, adp = mra.decode(fx["colors"])
        assert np.array_equal(ids, aov["id"]), m["name"]
        same(adp, np.abs(aov["dp"]), f"{m['name']}: colors.x is |dp|")
    assert (rendered["caustic"][1]["id"] < 0).any() and (rendered["complex"][1]["id"] < 0).any()
    cx = rendered["complex"][1]["id"]
    assert len(rendered["complex"][0]["spheres"]) == 783 and len(np.unique(cx[cx >= 0])) == 30
    fx = rendered["cornell_wrap"][0]
    kk = (26 + 25 * np.arange(fx["W"] * fx["H"], dtype=np.int64) + fx["sid"]) % 2 ** 32
    assert (kk < g.RAND_N - 5).any() and (kk >= g.RAND_N - 5).any()
    assert rendered["cornell_sid_last"][0]["sid"] == g.RAND_N - 1
    # the jitter matters: the unjittered rays differ from the jittered ones of the same scene
    assert (bits(rendered["cornell"][1]["dir"]) != bits(rendered["cornell_nojitter"][1]["dir"])).any()


@pytest.mark.parametrize("name", CASES)
def test_plane_identities(rendered, name):
    """normal == vnorm(position - p[id]) (device.cu:639-641, vec.h:22), dp == vdot(normal, dir) (:643),
    |dir| == 1 within 2 ulp, and the defined values on a miss.
    |dir|: dir = l * v with l = fl(1 / fl(sqrt(fl(v.v)))), u = 2^-24: the dot product is within 3u
    (relative), its root within 1.5u + u, the reciprocal adds u and the three component products
    at most u together -- 4.5u if every rounding went the same way, against the bound of
    2 ulp(1) = 4u; the roundings of the three components and of the dot product's terms never all
    align, so the bound holds with room (the largest deviation in the fixtures is 2.3u)."""
    fx, a = rendered[name]
    hit = a["id"] >= 0
    f32 = np.float32
    p = np.ascontiguousarray(fx["spheres"]["p"], f32)[np.where(hit, a["id"], 0)]
    v = a["position"] - p
    dot = v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        n = (f32(1) / np.sqrt(dot))[..., None] * v
    assert n.dtype == f32
    same(n[hit], a["normal"][hit], f"{name}: normal")
    nd = a["normal"] * a["dir"]
    same(((nd[..., 0] + nd[..., 1]) + nd[..., 2])[hit], a["dp"][hit], f"{name}: dp")
    assert (a["t"][hit] > 0.01).all()                                  # EPSILON (geom.h:6)
    length = np.sqrt((a["dir"].astype(np.float64) ** 2).sum(axis=-1))
    assert np.abs(length - 1.0).max() <= 2 * float(np.spacing(f32(1))), np.abs(length - 1.0).max()
    for k in ("t", "dp", "position", "normal"):
        assert (bits(a[k][~hit]) == 0).all(), f"{name}: {k} on a miss is not +0"
    assert a["id"].dtype == np.int32 and all(a[k].dtype == f32 for k in PLANES[1:])
    assert a["position"].shape == (fx["H"], fx["W"], 3) and a["t"].shape == (fx["H"], fx["W"])


@pytest.mark.skipif(not R.available(), reason="no reference build and no reference tree")
@pytest.mark.parametrize("name", CASES)
def test_fixture_regenerates(name):
    """Regenerating tests/golden/ref_aov_<name>.npz reproduces the committed bytes of every array."""
    lib = R.ref()
    case = {c["name"]: c for c in mra.cases()}[name]
    want = mra.fixture_arrays(case, mra.run_reference(case, lib, mra.table_of(case, lib, _TABLES)))
    have = np.load(os.path.join(GOLDEN, f"ref_aov_{name}.npz"))
    assert sorted(have.files) == sorted(want)
    for k, v in want.items():
        v = np.asarray(v)
        assert v.dtype == have[k].dtype and v.tobytes() == have[k].tobytes(), f"ref_aov_{name}.npz[{k}]"


_TABLES = {}


@pytest.mark.parametrize("name", ["cornell_glass", "caustic", "cornell_nojitter"])
def test_windows_and_pick_equal_slices(rendered, name):
    fx, whole = rendered[name]
    jitter = fx["table_seed"] >= 0
    with g.Renderer(fx["spheres"], fx["W"], fx["H"], g.Camera.from_buffer_copy(fx["camera"].tobytes()),
                    device=CPU) as r:
        if jitter:
            r.generate_rand(fx["table_seed"])
        assert_window_slices(r, whole, fx["sid"] if jitter else None,
                             [(7, 5, 9, 11), (3, 4, 1, 1), (19, 18, 1, 1), (0, 0, 20, 1), (19, 0, 1, 19)], name)
        ids = r.render_aov(window=(7, 5, 9, 11), planes=("id",))          # a partial request
        assert list(ids) == ["id"]


def test_errors():
    assert_errors(CPU)


def test_passes_after_render_aov_equal_passes_without_it():
    assert_non_interference(CPU, "cornell_glass", 33, 25)


def test_command_line_writes_npz_and_ppms(tmp_path):
    """python -m gpu_bidirectional_raytracer_amd.aov: sizes get +1, PREFIX.npz holds the six arrays
    of render_aov, --ppm adds the normal- and id-coloured images, --sid jitters on the seed-0 table."""
    from gpu_bidirectional_raytracer_amd import aov as cli
    scn = os.path.join(SCENES, "caustic.scn")
    prefix = str(tmp_path / "c")
    assert cli.main(["19", "18", scn, "--out", prefix, "--device", "-1", "--ppm"]) == 0
    got = np.load(prefix + ".npz")
    cam, sp = scene_of(scn, 20, 19)
    with g.Renderer(sp, 20, 19, cam, device=CPU) as r:
        want = r.render_aov()
        r.generate_rand(0)
        want7 = r.render_aov(sid=7)
    assert sorted(got.files) == sorted(PLANES)
    for k in PLANES:
        same(got[k], want[k], k)
    for name in ("c_normal.ppm", "c_id.ppm"):
        head = open(tmp_path / name).read(20).split()
        assert head[:4] == ["P3", "20", "19", "255"]
    rgba = cli.id_rgba(want)
    assert (rgba[want["id"] < 0, :3] == 0).all() and (rgba[want["id"] >= 0, :3] >= 64).all()
    assert cli.main(["19", "18", scn, "--out", prefix + "7", "--device", "-1", "--sid", "7"]) == 0
    same(np.load(prefix + "7.npz")["dir"], want7["dir"], "--sid 7")


def scene_of(path, W, H):
    cam, sp = g.read_scene(path)
    return g.update_camera(cam, W, H), sp


def test_pick_sphere_selects_and_reinitialises():
    """SmallPT.PickSphere on simple.scn: a hit selects the sphere and re-initialises as '+'/'-' do
    (display_func.c:336-343 -> ReInitScene); a miss changes nothing."""
    app = g.SmallPT(32, 24, os.path.join(SCENES, "simple.scn"), device=CPU)
    app.IdleFunc()
    app.IdleFunc(3)
    ids = app.renderer.render_aov()["id"]
    assert (ids < 0).any() and len(np.unique(ids[ids > 0])) >= 2
    before = (app.current_sphere, app.current_sample, app.flag, app.colors(), app.renderer.read_lightpaths())
    assert before[1] == 4 and before[2] == 2
    y, x = (int(v[0]) for v in np.nonzero(ids < 0))
    assert app.PickSphere(x, y) == -1
    after = (app.current_sphere, app.current_sample, app.flag, app.colors(), app.renderer.read_lightpaths())
    assert before[:3] == after[:3]
    same(before[3][0], after[3][0], "colors")
    assert np.array_equal(before[3][1], after[3][1]) and before[4].tobytes() == after[4].tobytes()
    want = int(np.unique(ids[ids > 0])[-1])
    y, x = (int(v[0]) for v in np.nonzero(ids == want))
    assert app.PickSphere(x, y) == want
    assert app.current_sphere == want and app.current_sample == 0 and app.flag == 2
    assert (app.colors()[1] == 0).all()                                # ReInitScene reset the counters
    g.sphere_key(app.spheres, app.current_sphere, "8")                 # the picked sphere is the one keys move
    app.FreeBuffers()
