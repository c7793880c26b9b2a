"""The named adversarial scenes (tests/adversarial_scenes.py) without a GPU: the reference says what
is right.  The oracle equals the reference's own code on every scene (light paths, colours, counters,
pixels), the CPU backend equals the oracle, every colour is finite; the scenes show what their names
promise (the higher twin on enough pixels, the lower on none); the host BVH builder classifies the
large scenes as stated and its traversal agrees with the every-sphere loops (tests/native/
bvh_check.cpp); and the host's black-surface exit proof (csrc/bdpt_util.c bdpt_zero_exit_safe)
returns what its own conditions imply.  Every comparison is on the float bits."""
import json
import os
import subprocess

import numpy as np
import pytest

import adversarial_scenes as A
import gpu_bidirectional_raytracer_amd as g
import oracle
from conftest import REPO
from oracle import ref as R

CPU = -1
W, H = 23, 17


@pytest.fixture(autouse=True)
def threads(monkeypatch):
    monkeypatch.setenv("BDPT_CPU_THREADS", "4")


@pytest.fixture(scope="module")
def rnd0():
    t = oracle.mt607(0)
    t.setflags(write=False)
    return t


def passes_of(name):
    return 6 if name in A.SMALL else 3


def schedule(n):
    s = g.PassScheduler()
    s.light()
    return s.next(n)


@pytest.fixture(scope="module")
def id_planes():
    """The CPU backend's un-jittered id plane of every scene at 45x31, once."""
    os.environ.setdefault("BDPT_CPU_THREADS", "4")
    out = {}
    for name in A.NAMES:
        cam, sp = A.scene(name)
        g.update_camera(cam, A.ID_W, A.ID_H)
        with g.Renderer(sp, A.ID_W, A.ID_H, cam, device=CPU) as r:
            out[name] = r.render_aov(planes=("id",))["id"]
    return out


def pixels_of(ids, k):
    return int((ids == k).sum())


@pytest.mark.parametrize("name", sorted(A.TWINS))
def test_twin_scenes_show_the_higher_twin_only(id_planes, name):
    ids = id_planes[name]
    cam, sp = A.scene(name)
    for grp in A.TWINS[name]:
        for k in grp[1:]:                                           # identical geometry, as the name says
            assert sp["rad"][k] == sp["rad"][grp[0]] and np.array_equal(sp["p"][k], sp["p"][grp[0]])
        assert pixels_of(ids, max(grp)) >= A.MIN_TWIN_PIXELS, (name, grp, pixels_of(ids, max(grp)))
        assert all(pixels_of(ids, k) == 0 for k in grp if k != max(grp)), (name, grp)


def test_twins_large_shows_enough_groups(id_planes):
    ids = id_planes["twins_large"]
    cam, sp = A.scene("twins_large")
    groups = A.twin_groups("twins_large")
    assert len(sp) == 180 and len(groups) == 43
    assert sorted(len(grp) for grp in groups) == [2, 2] + [4] * 40 + [9]
    seen = 0
    for grp in groups:
        for k in grp[1:]:
            assert sp["rad"][k] == sp["rad"][grp[0]] and np.array_equal(sp["p"][k], sp["p"][grp[0]])
        assert all(pixels_of(ids, k) == 0 for k in grp if k != max(grp)), grp
        seen += pixels_of(ids, max(grp)) > 0
    assert seen >= A.MIN_LARGE_GROUPS, seen
    spread = [max(grp) - min(grp) for grp in groups if len(grp) == 4]
    assert np.median(spread) > 60                                   # the permutation took the copies apart
    emits = sp["e"].any(axis=1)
    lo, hi = groups[41], groups[42]
    assert emits[min(lo)] and not emits[max(lo)] and not emits[min(hi)] and emits[max(hi)]
    assert int((sp["rad"] == 0).sum()) == 1


def test_other_scenes_mean_what_their_names_say(id_planes):
    ids = id_planes["tangent_chain"]
    assert all(pixels_of(ids, k) > 0 for k in A.CHAIN)
    cam, sp = A.scene("tangent_chain")
    for k in A.CHAIN[1:]:                                           # neighbours touch: centres 2 r apart
        assert np.linalg.norm(sp["p"][k].astype(np.float64) - sp["p"][k - 1]) == 2 * sp["rad"][k]
    assert sp["p"][10][1] == sp["rad"][10] and sp["p"][10][0] == sp["p"][2][0]      # on the floor wall's pole
    cam, sp = A.scene("light_touching_ceiling")
    d = np.linalg.norm(sp["p"][6].astype(np.float64) - sp["p"][3])
    assert d - sp["rad"][6] == sp["rad"][3] and sp["e"][6].any()                    # the two surfaces touch
    cam, sp = A.scene("wall_emitter")
    assert np.flatnonzero(sp["e"].any(axis=1)).tolist() == [4] and sp["rad"][4] == 1e4
    cam, sp = A.scene("camera_on_surface")
    o = np.array([cam.orig.x, cam.orig.y, cam.orig.z])
    assert np.linalg.norm(o - sp["p"][7]) == sp["rad"][7] and sp["refl"][7] == A.REFR
    cam, sp = A.scene("camera_inside_emitter")
    assert (cam.orig.x, cam.orig.y, cam.orig.z) == tuple(float(v) for v in sp["p"][6]) and sp["e"][6].any()
    assert (id_planes["camera_inside_emitter"] == 6).all()
    assert (id_planes["camera_along_up"] == -1).all()               # the reference's all-miss frame
    assert pixels_of(id_planes["zero_radius"], 7) == 0 and A.scene("zero_radius")[1]["rad"][7] == 0
    cam, sp = A.scene("concentric_glass")
    assert np.array_equal(sp["p"][7], sp["p"][8]) and np.array_equal(sp["p"][7], sp["p"][9])
    assert sp["rad"][9] == np.nextafter(np.float32(14), np.float32(np.inf)) and sp["rad"][7] == 14
    assert (A.scene("neg_radius")[1]["rad"][7:] < 0).all() and A.scene("neg_radius_emitter")[1]["rad"][6] == -6
    assert all(len(A.scene(n)[1]) <= 16 for n in A.SMALL)           # the specialised kernels unroll them
    for n, (tree, brute) in A.CLASSES.items():
        assert len(A.scene(n)[1]) == tree + brute


@pytest.fixture(scope="module")
def oracle_frames(rnd0):
    """(lp, colors, counter, pixels) of the oracle per scene at 23x17, computed on first use."""
    cache = {}

    def get(name):
        if name not in cache:
            cam, sp = A.scene(name)
            g.update_camera(cam, W, H)
            sid, vlp = schedule(passes_of(name))
            lp = oracle.light_pass(sp, rnd0, 0)
            cache[name] = (lp,) + tuple(oracle.path_passes(sp, rnd0, cam, W, H, lp, sid, vlp))
        return cache[name]
    return get


@pytest.mark.skipif(not R.available(), reason="no reference build and no reference tree")
@pytest.mark.parametrize("name", A.NAMES)
def test_oracle_equals_reference(rnd0, name):
    from test_ref_parity import assert_frame_equal, both
    cam, sp = A.scene(name)
    g.update_camera(cam, W, H)
    sid, vlp = schedule(passes_of(name))
    o, r = both(R.ref(), sp, rnd0, oracle.camera_array(cam), W, H, sid, vlp)
    assert_frame_equal(o, r, name)
    assert (r[2] == len(sid)).all()


@pytest.mark.parametrize("name", A.NAMES)
def test_cpu_backend_equals_oracle(oracle_frames, name):
    cam, sp = A.scene(name)
    g.update_camera(cam, W, H)
    sid, vlp = schedule(passes_of(name))
    with g.Renderer(sp, W, H, cam, device=CPU) as r:
        r.light_pass(0)
        r.path_passes(sid, vlp)
        col, cnt = r.read_radiance()
        px = r.read_pixels()
        lp = r.read_lightpaths()
    olp, ocol, ocnt, opx = oracle_frames(name)
    assert np.isfinite(ocol).all(), f"{name}: the oracle's colours are not all finite"
    assert lp.tobytes() == olp.tobytes(), f"{name}: light paths differ"
    assert np.array_equal(cnt, ocnt)
    bad = int((col.view(np.uint32) != ocol.view(np.uint32)).sum())
    assert bad == 0, f"{name}: {bad} colour values differ"
    assert np.array_equal(px, opx)


@pytest.fixture(scope="module")
def bvh_check_exe(tmp_path_factory):
    """tests/native/bvh_check.cpp, built as test_bvh_margin.py builds it."""
    d = tmp_path_factory.mktemp("bvh_check")
    hipcc = "/opt/rocm/bin/hipcc"
    flags = ["-O2", "-fPIC", "-ffp-contract=off", "-std=c++17"]
    objs = []
    for src in ("tests/native/bvh_check.cpp", "gpu_bidirectional_raytracer_amd/csrc/bdpt_bvh.cpp"):
        obj = str(d / (os.path.basename(src) + ".o"))
        subprocess.check_call([hipcc, *flags, "-c", os.path.join(REPO, src), "-o", obj])
        objs.append(obj)
    util = str(d / "bdpt_util.o")
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-ffp-contract=off", "-c",
                           os.path.join(REPO, "gpu_bidirectional_raytracer_amd/csrc/bdpt_util.c"), "-o", util])
    exe = str(d / "bvh_check")
    subprocess.check_call(["g++", "-o", exe, *objs, util, "-lm"])
    return exe


@pytest.mark.parametrize("name", ["twins_large", "many_big", "min_tree_24", "min_tree_23"])
def test_host_bvh_classifies_and_traverses(bvh_check_exe, tmp_path, name):
    """The scene through a .scn file (which must round-trip every bit) and bvh_check's 100k rays."""
    cam, sp = A.scene(name)
    path = str(tmp_path / (name + ".scn"))
    A.write_scn(path, cam, sp)
    cam2, sp2 = g.read_scene(path)
    assert sp2.tobytes() == sp.tobytes() and (cam2.orig.z, cam2.target.y) == (cam.orig.z, cam.target.y)
    out = subprocess.run([bvh_check_exe, path, "100000", "5"], capture_output=True, text=True)
    rec = json.loads(out.stdout)
    print(name, rec)
    tree, brute = A.CLASSES[name]
    if not tree:
        assert out.returncode == 0 and rec == {"bvh": False}
        return
    assert out.returncode == 0 and rec["bvh"], (name, out.stdout, out.stderr)
    assert (rec["bvh_spheres"], rec["walls"]) == (tree, brute), rec
    assert rec["bad_closest"] == 0 and rec["bad_shadow"] == 0 and rec["rays"] == 100000, rec
    assert rec["hits"] > 50000


def zero_exit(sp):
    sp = g.spheres_to_array(sp)
    return int(g.lib.bdpt_zero_exit_safe(g._sphere_ptr(sp), len(sp)))


def test_black_surface_exit_proof():
    """bdpt_zero_exit_safe by its own conditions: a black non-emitter must exist, every radius must
    be above 2^-16 of the scene's scale, and every emitter must keep a gap of max(1, 1e-4 scale)
    (= 2 for walls of 1e4) from every other surface, inside or outside."""
    floor_only = A.box()
    for w in floor_only:
        w[3][:] = 0.75                                              # no black wall: the ball decides
    ball = A.S(8, (30, 20, 60), c=A.BLACK)
    plain = floor_only + [A.light(), ball]
    assert zero_exit(A.pack(plain)) == 1
    assert zero_exit(A.pack(floor_only + [A.light(), A.S(8, (30, 20, 60), c=A.RED)])) == 0     # nothing black
    assert zero_exit(A.scene("twin_black_emitter")[1]) == 0
    assert zero_exit(A.scene("light_touching_ceiling")[1]) == 0
    assert zero_exit(A.pack(floor_only + [A.light(p=(50, 74, 80)), ball])) == 0               # touching a wall
    assert zero_exit(A.pack(floor_only + [A.light(p=(50, 73.5, 80)), ball])) == 0             # 0.5 from it
    assert zero_exit(A.pack(floor_only + [A.light(p=(50, 71.5, 80)), ball])) == 1             # 2.5 from it
    shell = A.S(6.5, A.L_P, c=A.WHITE, refl=A.REFR)
    assert zero_exit(A.pack(floor_only + [A.light(), shell, ball])) == 0                      # in a glass shell
    assert zero_exit(A.pack(plain + [A.S(0, (50, 44, 160))])) == 0                            # a radius-0 sphere
    assert zero_exit(A.scene("zero_radius")[1]) == 0
    # a negative radius: the gap and the size bounds take fabs(rad), the sphere test squares it, so
    # the proof holds as for +6 and the scene is accepted
    assert zero_exit(A.pack(floor_only + [A.light(rad=-6.0), ball])) == 1
    assert zero_exit(A.scene("neg_radius_emitter")[1]) == 1
    assert zero_exit(A.pack(floor_only + [A.light(p=(50, 74, 80), rad=-6.0), ball])) == 0
