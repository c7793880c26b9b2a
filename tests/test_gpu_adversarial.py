"""The named adversarial scenes (tests/adversarial_scenes.py) through the HIP kernels, bit for bit
against the oracle (which tests/test_adversarial_cpu.py holds to the reference's own code on the
same scenes): hit-distance ties, touching and concentric spheres, emitters that share their geometry
with a non-emitter or touch a wall, an emitter wall, negative and zero radii, degenerate cameras, and
scenes on the BVH builder's classification limits.  These reach what the seeded random scenes of
test_gpu_fuzz.py never do: the tie rule (the higher index wins at equal distance, device.cu:106-124)
in the generic loop, in the specialised kernels' integer keys, in the BVH walk across the brute list
and the tree, and in the first-hit kernel's copies of them; and the exact shortcuts of the
specialised kernels that reason about where the emitters are.  Last, the scene-size limit of the
brute-force kernels: the largest scene whose tables fit a workgroup's LDS renders, the next one is
refused before anything is launched.  No tolerance anywhere."""
import numpy as np
import pytest

import adversarial_scenes as A
import gpu_bidirectional_raytracer_amd as g
import oracle
from aov_common import PLANES, bits, probe_colors, same, same_aov
from make_ref_aov_golden import probe_scene

pytestmark = pytest.mark.gpu

CPU = -1
SMALL_WH, LARGE_WH = (45, 31), (33, 25)
SID = 7
TREES = [n for n in A.LARGE if A.CLASSES[n][0]]
LARGE_CASES = [(n, t) for n in A.LARGE for t in ("bvh", "brute") if t == "brute" or n in TREES]


def size_of(name):
    return SMALL_WH if name in A.SMALL else LARGE_WH


def schedule(n):
    s = g.PassScheduler()
    s.light()
    return s.next(n)


@pytest.fixture(scope="module")
def rnd0():
    t = oracle.mt607(0)
    t.setflags(write=False)
    return t


@pytest.fixture(scope="module")
def light_paths(rnd0):
    """The oracle's light paths per scene, computed on first use and never modified."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = oracle.light_pass(A.scene(name)[1], rnd0, 0)
            cache[name].setflags(write=False)
        return cache[name]
    return get


@pytest.fixture(scope="module")
def oracle_frames(rnd0, light_paths):
    """(colors, counter, pixels) of the oracle per (scene, passes) at the scene's frame size."""
    cache = {}

    def get(name, npass):
        if (name, npass) not in cache:
            W, H = size_of(name)
            cam, sp = A.scene(name)
            g.update_camera(cam, W, H)
            sid, vlp = schedule(npass)
            cache[name, npass] = oracle.path_passes(sp, rnd0, cam, W, H, light_paths(name), sid, vlp)
        return cache[name, npass]
    return get


def assert_frame(r, want, what):
    col, cnt = r.read_radiance()
    ocol, ocnt, opx = want
    assert np.array_equal(cnt, ocnt), f"{what}: counters differ"
    bad = int((bits(col) != bits(ocol)).sum())
    assert bad == 0, f"{what}: {bad} of {col.size} colour values differ"
    assert np.array_equal(r.read_pixels(), opx), f"{what}: pixels differ"


def make(name, gpu):
    W, H = size_of(name)
    cam, sp = A.scene(name)
    g.update_camera(cam, W, H)
    return g.Renderer(sp, W, H, cam, device=gpu), cam, sp


# ---- the light pass ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", A.NAMES)
def test_light_pass_equals_oracle(gpu, light_paths, name):
    """bdpt_light_kernel on the twin, wall and negative-radius emitters (and every other scene)."""
    r, cam, sp = make(name, gpu)
    assert A.has_emitter(sp)
    with r:
        r.light_pass(0)
        lp = r.read_lightpaths()
    want = light_paths(name)
    diff = int((lp.view(np.uint32).reshape(len(lp), -1) != want.view(np.uint32).reshape(len(lp), -1)).any(axis=1).sum())
    assert diff == 0, f"{name}: {diff} of {len(lp)} light paths differ"


# ---- the path kernels ---------------------------------------------------------------------------

@pytest.mark.parametrize("specialize", [True, False])
@pytest.mark.parametrize("streams", [0, 1])
@pytest.mark.parametrize("name", A.SMALL)
def test_small_scene_bit_exact(gpu, oracle_frames, name, streams, specialize):
    r, cam, sp = make(name, gpu)
    with r:
        r.set_specialize(specialize)
        r.set_streams(streams)
        r.light_pass(0)
        sid, vlp = schedule(6)
        r.path_passes(sid, vlp)
        assert r.last_specialized == specialize, r.specialize_status
        assert r.last_traversal == "brute"
        if name == "twin_black_emitter":                    # an emitter inside a black surface: no exit proof
            assert "zero_exit" not in r.last_features
        assert_frame(r, oracle_frames(name, 6), f"{name} streams {streams} specialize {specialize}")


@pytest.mark.parametrize("name,traversal", LARGE_CASES)
def test_large_scene_bit_exact(gpu, oracle_frames, name, traversal):
    r, cam, sp = make(name, gpu)
    with r:
        assert r.has_bvh == (name in TREES)
        r.set_traversal(traversal)
        r.light_pass(0)
        sid, vlp = schedule(4)
        r.path_passes(sid, vlp)
        assert r.last_traversal == traversal
        assert_frame(r, oracle_frames(name, 4), f"{name} {traversal}")


@pytest.mark.parametrize("name,want", [("auto_127", "brute"), ("auto_128", "bvh")])
def test_auto_traversal_switches_at_128(gpu, oracle_frames, name, want):
    r, cam, sp = make(name, gpu)
    with r:
        assert r.has_bvh
        r.light_pass(0)
        sid, vlp = schedule(4)
        r.path_passes(sid, vlp)
        assert r.last_traversal == want
        assert_frame(r, oracle_frames(name, 4), f"{name} auto")


@pytest.mark.parametrize("name", ["twin_diff_spec", "twins_large"])
def test_call_sequence_bit_exact(gpu, rnd0, light_paths, name):
    """Five calls of 1-20 passes in the auto stream mode (as test_gpu_fuzz's call sequences): the
    tie code through the pooled, units and fused variants that auto measures, one frame throughout."""
    rng = np.random.default_rng(5000 + len(name))
    W, H = size_of(name)
    r, cam, sp = make(name, gpu)
    with r:
        r.set_streams(0)
        r.light_pass(0)
        s = g.PassScheduler()
        s.light()
        ocol = ocnt = None
        for call in range(5):
            n = int(rng.integers(1, 21))
            sid, vlp = s.next(n)
            r.path_passes(sid, vlp)
            ocol, ocnt, opx = oracle.path_passes(sp, rnd0, cam, W, H, light_paths(name), sid, vlp,
                                                 colors=ocol, counter=ocnt)
            assert_frame(r, (ocol, ocnt, opx), f"{name} call {call} ({n} passes, S={r.last_streams})")


# ---- the first hit ------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cpu_planes():
    """The CPU backend's planes per scene, jittered (table seed 15, sid 7) and not."""
    cache = {}

    def get(name):
        if name not in cache:
            W, H = size_of(name)
            cam, sp = A.scene(name)
            g.update_camera(cam, W, H)
            with g.Renderer(sp, W, H, cam, device=CPU) as r:
                r.generate_rand(15)
                cache[name] = {True: r.render_aov(sid=SID), False: r.render_aov()}
        return cache[name]
    return get


def same_planes(got, want, what, nan_dir):
    """All planes on their bits; with a degenerate camera basis the ray directions are NaN, whose
    sign and payload are not comparable between a CPU and a GPU: there only which entries are NaN."""
    if not nan_dir:
        same_aov(got, want, what)
        return
    for k in PLANES:
        if k == "dir":
            assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])), f"{what}: dir NaN entries"
            fin = ~np.isnan(want[k])
            same(got[k][fin], want[k][fin], f"{what}: dir where finite")
        else:
            same(got[k], want[k], f"{what}: {k}")


@pytest.mark.parametrize("name", A.NAMES)
def test_first_hit_equals_cpu_backend(gpu, cpu_planes, name):
    want = cpu_planes(name)
    r, cam, sp = make(name, gpu)
    with r:
        r.generate_rand(15)
        for traversal in (("brute", "bvh") if name in TREES else ("brute",)):
            r.set_traversal(traversal)
            for jitter in (True, False):
                aov = r.render_aov(sid=SID if jitter else None)
                assert r.last_aov_traversal == traversal
                same_planes(aov, want[jitter], f"{name} {traversal} jitter={jitter}", name == "camera_along_up")
        ids = want[False]["id"]
        for grp in A.twin_groups(name):                     # the centre pixel of each visible twin
            ys, xs = np.nonzero(ids == max(grp))
            if not len(ys):
                continue
            k = int(np.argmin((ys - ys.mean()) ** 2 + (xs - xs.mean()) ** 2))
            for traversal in (("brute", "bvh") if name in TREES else ("brute",)):
                r.set_traversal(traversal)
                i, t = r.pick(int(xs[k]), int(ys[k]))
                assert i == max(grp), f"{name} {traversal}: pick({xs[k]}, {ys[k]}) = {i}, twins {grp}"
                assert np.float32(t).view(np.uint32) == bits(want[False]["t"])[ys[k], xs[k]]
    if name in A.TWINS:
        assert all((ids == max(grp)).sum() >= A.MIN_TWIN_PIXELS for grp in A.TWINS[name])


@pytest.mark.parametrize("traversal", ["brute", "bvh"])
@pytest.mark.parametrize("name", ["twin_diff_spec", "twins_large"])
def test_path_kernel_of_the_same_context_agrees(gpu, name, traversal):
    """The self-probe of test_gpu_aov.py: one path pass over the all-emitter copy of the scene
    returns e[id] * |dp| of the path kernel's own first hit, and render_aov gives the same -- at a
    tie both must have taken the same twin.  (twin_diff_spec has no tree: both modes scan.)"""
    W, H = size_of(name)
    cam, sp = A.scene(name)
    sp = probe_scene(sp)
    g.update_camera(cam, W, H)
    with g.Renderer(sp, W, H, cam, device=gpu) as r:
        r.set_traversal(traversal)
        r.light_pass(3)                                     # table seed 15
        aov = r.render_aov(sid=SID)
        r.path_passes([SID], [1])
        col, cnt = r.read_radiance()
        assert r.last_traversal == r.last_aov_traversal == (traversal if name in TREES else "brute")
    assert (cnt == 1).all()
    same(probe_colors(sp, aov), col, f"{name} {traversal}: e[id] * |dp| vs the path kernel's radiance")
    tops = [max(grp) for grp in A.twin_groups(name)]
    assert np.isin(aov["id"], tops).sum() >= 20


# ---- the scene-size limit ------------------------------------------------------------------------
# A brute-force launch keeps 5 float4 per sphere in LDS (4 tables and the non-emitters' list,
# bdpt_plan.h bdpt_path_smem), next to what the kernel declares itself; the sum must fit the
# device's LDS per workgroup.  Frame 16x8, 2 passes.

LW, LH = 16, 8
PER_SPHERE = 16 * 5


def lds_frame(sp, cam, rnd0):
    sid, vlp = schedule(2)
    return sid, vlp, oracle.path_passes(sp, rnd0, cam, LW, LH, oracle.light_pass(sp, rnd0, 0), sid, vlp)


def brute_n_max(gpu, streams):
    """The largest big_brute scene the brute-force kernel takes with this stream setting, from the
    launch's own figures on a small scene of the same kind: dynamic LDS grows by PER_SPHERE bytes
    per sphere (one emitter throughout), the rest is the same launch."""
    n0 = 200
    cam, sp = A.big_brute(n0)
    g.update_camera(cam, LW, LH)
    with g.Renderer(sp, LW, LH, cam, device=gpu) as r:
        r.set_traversal("brute")
        r.set_streams(streams)
        r.light_pass(0)
        r.path_passes(*schedule(2))
        lds = r.path_lds()
    assert lds["limit"] >= 64 * 1024 and 0 < lds["static"] < 16 * 1024 and lds["dynamic"] > PER_SPHERE * n0
    return n0 + (lds["limit"] - lds["static"] - lds["dynamic"]) // PER_SPHERE, lds


@pytest.mark.parametrize("streams", [0, 1])
def test_largest_brute_scene_renders_and_the_next_is_refused(gpu, rnd0, streams):
    n_max, lds0 = brute_n_max(gpu, streams)
    print(f"streams {streams}: static {lds0['static']} B, limit {lds0['limit']} B, n_max {n_max}")
    assert 1000 < n_max < 2100
    cam, sp = A.big_brute(n_max)
    g.update_camera(cam, LW, LH)
    assert int((sp[7:][49::50]["p"] == sp[7:][48::50]["p"]).all(axis=1).sum()) == (n_max - 7) // 50   # the copies
    with g.Renderer(sp, LW, LH, cam, device=gpu) as r:
        r.set_traversal("brute")
        r.set_streams(streams)
        r.light_pass(0)
        sid, vlp, want = lds_frame(sp, cam, rnd0)
        r.path_passes(sid, vlp)
        lds = r.path_lds()
        assert lds["static"] == lds0["static"]                          # the same kernel as the small scene's
        assert lds["static"] + lds["dynamic"] <= lds["limit"] < lds["static"] + lds["dynamic"] + PER_SPHERE
        assert r.last_traversal == "brute"
        assert_frame(r, want, f"big_brute({n_max}) streams {streams}")
        # one sphere more: refused before anything is launched, the frame stays, the context lives
        cam1, sp1 = A.big_brute(n_max + 1)
        r.set_scene(sp1)
        r.light_pass(0)
        before = r.read_radiance()
        with pytest.raises(g.BdptError, match="too large for LDS") as e:
            r.path_passes(sid, vlp)
        assert e.value.code == g._lib.BDPT_EINVAL
        lds1 = r.path_lds()                                             # the refused launch's figures
        assert lds1["static"] == lds["static"] and lds1["dynamic"] == lds["dynamic"] + PER_SPHERE
        assert lds1["static"] + lds1["dynamic"] > lds1["limit"]
        after = r.read_radiance()
        assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()
        cam2, sp2 = A.scene("twin_diff_spec")
        g.update_camera(cam2, LW, LH)
        r.set_camera(cam2)
        r.set_scene(sp2)
        r.reset_accum()
        r.light_pass(0)
        r.path_passes(sid, vlp)
        assert_frame(r, lds_frame(sp2, cam2, rnd0)[2], "twin_diff_spec after the refused call")


def test_scene_past_the_brute_limit_renders_on_the_tree(gpu, rnd0):
    """The way out the refusal leaves: the same kind of scene, 200 spheres past the limit, has a
    tree, and the BVH kernel stages only the brute list (the walls)."""
    n_max, _ = brute_n_max(gpu, 0)
    cam, sp = A.big_brute(n_max + 200)
    g.update_camera(cam, LW, LH)
    with g.Renderer(sp, LW, LH, cam, device=gpu) as r:
        assert r.has_bvh
        r.set_traversal("bvh")
        r.light_pass(0)
        sid, vlp, want = lds_frame(sp, cam, rnd0)
        r.path_passes(sid, vlp)
        assert r.last_traversal == "bvh"
        lds = r.path_lds()
        assert lds["static"] + lds["dynamic"] < 32 * 1024
        assert_frame(r, want, f"big_brute({n_max + 200}) on the tree")
        r.set_traversal("brute")
        with pytest.raises(g.BdptError, match="too large for LDS") as e:
            r.path_passes(sid, vlp)
        assert e.value.code == g._lib.BDPT_EINVAL
