"""The scenes and rules of tests/count_scenes.py, on the CPU: what tests/test_gpu_sphere_counts.py
relies on when it runs the path kernels across sphere counts and emitter positions.

  * The Python restatement of the compile-time rules equals the C++ (bdpt_jit_plan.h vac_list, and
    the part-full rounds' pf_iters / pf_fits as tests/native/jit_plan_check.cpp quotes them; the
    quotation and the run-time choice of lg are held to the text of csrc/bdpt_kernels.hip).
  * CASES covers every class a build can have (count_scenes.UNIVERSE) and the counts 1, 2, 16, 17,
    32, 33, 63 and 64, and no case can go without losing one.
  * Every scene is well posed: the CPU backend equals the oracle bit for bit at 45 x 31 after 4
    passes (those of the precompiled kernels' test), nothing is NaN, and a scene with an emitter is not black.
  * The tiny frames: under the jitter of every pass of the schedule, every pixel's first hit is a
    coloured diffuse non-emitter (the CPU backend's render_aov).  Such a pixel queues, at its
    first vertex, the first emitter's NEE ray and the VLP ray, and one NEE ray per further emitter,
    so a wave's rounds there have at most c = 2 * pixels and c = pixels rays, and with
    count_scenes.round_lg (before the reduction `while 2^(lg - 1) >= nl`):

        frame    pixels   first step: c, lg    further emitters: c, lg
        1 x 1       1          2   5                  1   5
        2 x 1       2          4   4                  2   5
        4 x 1       4          8   3                  4   4
        8 x 1       8         16   2                  8   3
        8 x 2      16         32   1                 16   2
        8 x 4      32         64   0 (full)          32   1

    (test_tiny_frame_lg derives the table; count_scenes.MORE_TINY adds 1 x 2, 3 x 1 and 2 x 2).  Later vertices queue fewer rays, as paths end, and
    reach the higher lg again.  Scenes without an emitter or without a non-emitter queue no ray.
  * Sensitivity: for every witness emitter (index >= 32, index n - 1, or in a masked tail) the
    45 x 31 frame has at least MIN_TWIN_PIXELS (pixel, pass) pairs whose VLP ray -- from the
    pixel's first hit to the pass's light point, facing both ways -- crosses that emitter and no
    non-emitter, by float64 segment tests: pixels that change if the emitter's mask bit is lost.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import count_scenes as cs
import gpu_bidirectional_raytracer_amd as g
from accum_modes import same
from adversarial_scenes import MIN_TWIN_PIXELS
from conftest import REPO

HIPCC = "/opt/rocm/bin/hipcc"
KERNELS = os.path.join(REPO, "gpu_bidirectional_raytracer_amd", "csrc", "bdpt_kernels.hip")
CHECK = os.path.join(REPO, "tests", "native", "jit_plan_check.cpp")
W, H = cs.FULL_FRAME
ALL = list(dict.fromkeys(cs.CASES + cs.PRECOMPILED))
EPS = 0.01                                                  # EPSILON of the shadow rays' maxt


# ---- the restatement ------------------------------------------------------------------------

@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_rules_equal_the_cpp(tmp_path):
    exe = tmp_path / "jit_plan_check"
    subprocess.check_call([HIPCC, "-O1", "-std=c++17", "-o", str(exe), CHECK])
    out = subprocess.run([str(exe), "rules"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0
    vac, pf = {}, {}
    for line in out.stdout.split("\n"):
        f = line.split()
        if f and f[0] == "vac":
            vac[(int(f[1]), int(f[2]))] = bool(int(f[3]))
        elif f and f[0] == "pf":
            pf[(int(f[1]), int(f[2]))] = (bool(int(f[3])), int(f[4]))
    assert len(vac) == sum(n + 1 for n in range(1, 65)) and len(pf) == 64 * 5
    for (n, n_vac), v in vac.items():
        assert cs.vac_list(n, n_vac) == v, (n, n_vac)
    for (nl, lg), v in pf.items():
        assert (cs.pf_fits(nl, lg), cs.pf_iters(nl, lg)) == v, (nl, lg)


def test_quoted_rules_are_the_kernel_source():
    """The lines jit_plan_check.cpp quotes stand in bdpt_kernels.hip word for word, and so does the
    run-time choice of lg that round_lg restates."""
    src = open(KERNELS).read()
    quoted = [ln for ln in open(CHECK).read().split("\n")
              if ln.startswith(("constexpr int pf_iters", "constexpr bool pf_fits", "#define BDPT_PF_MAX_IT"))]
    assert len(quoted) == 3
    for ln in quoted:
        assert src.count(ln + "\n") == 1, ln
    assert cs.PF_MAX_IT == int(re.search(r"#define BDPT_PF_MAX_IT (\d+)", src).group(1))
    assert "int lg = c <= 2 ? 5 : c <= 4 ? 4 : c <= 8 ? 3 : (c <= 16 ? 2 : (c <= 32 ? 1 : 0));\n" in src
    assert "while (lg > 0 && (1 << (lg - 1)) >= nl) lg--;\n" in src
    for nl in range(1, 65):
        for c in range(1, 65):
            lg = 5 if c <= 2 else 4 if c <= 4 else 3 if c <= 8 else 2 if c <= 16 else 1 if c <= 32 else 0
            while lg > 0 and (1 << (lg - 1)) >= nl:
                lg -= 1
            assert cs.round_lg(c, nl) == lg
            assert lg == 0 or (1 << (lg - 1)) < nl          # the lists that pf_fits says reach lg


def test_tiny_frame_lg():
    """The table of the module docstring."""
    want = {(1, 1): (2, 5, 1, 5), (2, 1): (4, 4, 2, 5), (4, 1): (8, 3, 4, 4), (8, 1): (16, 2, 8, 3),
            (8, 2): (32, 1, 16, 2), (8, 4): (64, 0, 32, 1)}
    assert list(want) == cs.TINY_FRAMES
    for (w, h), (c0, lg0, c1, lg1) in want.items():
        assert (cs.frame_rays(w, h), cs.frame_rays(w, h, 1)) == (c0, c1)
        assert (cs.round_lg(c0, 64), cs.round_lg(c1, 64)) == (lg0, lg1)
    assert [cs.round_lg(cs.frame_rays(w, h), 64) for w, h in cs.MORE_TINY] == [4, 3, 3]
    # together the first steps reach every group count of every list that has it
    for nl in range(2, 65):
        reached = {cs.round_lg(cs.frame_rays(w, h, s), nl) for w, h in cs.TINY_FRAMES for s in (0, 1)}
        assert reached >= {lg for lg in range(1, 6) if (1 << (lg - 1)) < nl}


# ---- coverage -------------------------------------------------------------------------------

def _covered(cases):
    out = set()
    for c in cases:
        out |= cs.classes(*c)
    return out


def test_cases_cover_every_class():
    assert _covered(cs.CASES) == cs.UNIVERSE
    assert {n for n, _ in cs.CASES} >= set(cs.REQUIRED_N)
    assert len(set(cs.CASES)) == len(cs.CASES)
    # the universe holds what the issue names: every kind at every lg, both mask widths, ...
    kinds = {(c[1], c[2]) for c in cs.UNIVERSE if c[0] == "all"}
    assert kinds == {(lg, k) for lg in range(1, 6) for k in ("exact", "tail")} | {(1, "loop"), (2, "loop")}
    for c in [("mask", 32), ("mask", 64), ("emitter@", 32), ("emitter@", 63), ("vac_list", True), ("vac_list", False),
              ("n_vac=0",), ("no_emitter",), ("tail_lit", 5, "wide"), ("tail_dark", 5, "wide"), ("vac", 1, "loop", "wide")]:
        assert c in cs.UNIVERSE, c


@pytest.mark.parametrize("case", cs.CASES, ids=cs.case_id)
def test_no_case_can_go(case):
    rest = [c for c in cs.CASES if c != case]
    lost = cs.UNIVERSE - _covered(rest)
    alone = case[0] in cs.REQUIRED_N and case[0] not in {n for n, _ in rest}
    print(f"{cs.case_id(case)}: alone brings {sorted(lost, key=str)}{' and its count' if alone else ''}")
    assert lost or alone


def test_plan_of_the_boundaries():
    """16 / 17 and 32 / 33, where pf_fits and the mask change."""
    assert cs.pf_fits(16, 1) and not cs.pf_fits(17, 1) and cs.pf_fits(32, 2) and not cs.pf_fits(33, 2)
    assert ("all", 1, "exact", "narrow") in cs.classes(16, (15,)) and ("all", 1, "loop", "narrow") in cs.classes(17, (16,))
    assert ("mask", 32) in cs.classes(32, (31,)) and ("mask", 64) in cs.classes(33, (0,))
    assert cs.witnesses(33, (0,)) == [] and cs.witnesses(64, (8, 32, 33, 63)) == [32, 33, 63]
    assert cs.witnesses(17, (16,)) == [16] and cs.witnesses(1, (0,)) == []


# ---- the scenes -----------------------------------------------------------------------------

@pytest.mark.parametrize("case", ALL, ids=cs.case_id)
def test_scene_is_what_it_says(case):
    n, em = case
    cam, sp = cs.scene(*case)
    assert len(sp) == n and np.flatnonzero(sp["e"].any(axis=1)).tolist() == sorted(em)
    walls = np.flatnonzero(sp["rad"] >= 1e3)
    assert len(walls) == (6 if n >= 8 else min(6, n - len(em)))
    small = np.flatnonzero(sp["rad"] < 1e3)
    p, r = sp["p"][small].astype(np.float64), sp["rad"][small].astype(np.float64)
    d = np.linalg.norm(p[:, None] - p[None], axis=-1) - r[:, None] - r[None]
    assert (d[np.triu_indices(len(small), 1)] > 0.25).all(), "small spheres overlap"
    if n > len(em):                                          # inside the room, off the walls, above the view
        assert (p[:, 1] - r >= cs.CAM_O[1] - 0.14 * (cs.CAM_O[2] - p[:, 2]) + 1.0).all()
        assert (p[:, 1] + r < 80).all() and (p[:, 0] - r > 0).all() and (p[:, 0] + r < 100).all()
    again = cs.scene(*case)[1]
    assert again.tobytes() == sp.tobytes()                   # seeded
    if n >= 8 and n - 1 not in em:
        last = cs.scene(n, em, wall_last=True)[1]
        assert last["rad"][n - 1] >= 1e3 and np.flatnonzero(last["e"].any(axis=1)).tolist() == sorted(em)


def _state(r):
    col, cnt = r.read_radiance()
    return col, cnt, r.read_pixels()


@pytest.mark.parametrize("case", ALL, ids=cs.case_id)
def test_cpu_backend_equals_oracle(case):
    cam, sp = cs.load(case, W, H)
    sid, vlp = cs.schedule(cs.SHORT)
    with g.Renderer(sp, W, H, cam, device=-1) as r:
        r.light_pass(0)
        r.path_passes(sid, vlp)
        got = _state(r)
        lp = r.read_lightpaths()
    want = cs.expected(case, W, H, cs.SHORT)
    for a, b, what in zip(got, want, ("colors", "counter", "pixels")):
        same(a, b, f"{cs.case_id(case)}: {what}")
    same(lp.view(np.float32), cs.light_points(case).view(np.float32), f"{cs.case_id(case)}: light points")
    assert not np.isnan(got[0]).any() and not np.isnan(lp.view(np.float32)).any()
    if case[1]:
        assert got[0].max() > 0, "an emitter and a black frame"


def _lit_diffuse(sp):
    """Spheres a path goes on from with shadow rays: diffuse, no emitter, not black (the kernels
    may end a path at a black surface)."""
    return (sp["refl"] == g.DIFF) & ~sp["e"].any(axis=1) & sp["c"].any(axis=1)


@pytest.fixture(scope="module")
def cpu_frames():
    """One CPU context per frame size, table of seed 0, re-used across the scenes."""
    ctx = {}

    def get(width, height, cam, sp):
        if (width, height) not in ctx:
            ctx[(width, height)] = g.Renderer(sp, width, height, cam, device=-1)
            ctx[(width, height)].generate_rand(0)
        r = ctx[(width, height)]
        r.set_scene(sp)
        r.set_camera(cam)
        return r
    yield get
    for r in ctx.values():
        r.close()


@pytest.mark.parametrize("case", [c for c in cs.CASES if c[1] and len(c[1]) < c[0]], ids=cs.case_id)
def test_tiny_frames_start_at_lit_diffuse_surfaces(case, cpu_frames):
    sid, _ = cs.schedule(cs.NPASS)
    for w, h in cs.TINY_FRAMES + cs.MORE_TINY + [cs.FULL_FRAME]:
        cam, sp = cs.load(case, w, h)
        ok = _lit_diffuse(sp)
        r = cpu_frames(w, h, cam, sp)
        for s in sid:
            ids = r.render_aov(sid=int(s), planes=("id",))["id"]
            assert (ids >= 0).all() and ok[ids].all(), f"{cs.case_id(case)} {w}x{h} sid {s}: first hits {np.unique(ids)}"


def _crossed(p, d, maxt, sp):
    """[pixels, spheres]: the shadow ray p + t d, EPS < t < maxt, crosses the sphere (float64)."""
    c, rad = sp["p"].astype(np.float64), sp["rad"].astype(np.float64)
    op = c[None] - p[:, None]
    b = (op * d[:, None]).sum(-1)
    det = b * b - (op * op).sum(-1) + rad[None] ** 2
    root = np.sqrt(np.maximum(det, 0))
    t = np.where(b - root > EPS, b - root, b + root)
    return (det >= 0) & (t > EPS) & (t < maxt[:, None])


def witness_pairs(case, passes, cpu_frames):
    """{witness emitter: (pixel, pass) pairs of the 45 x 31 frame whose VLP ray exists, crosses it
    and crosses no non-emitter}."""
    cam, sp = cs.load(case, W, H)
    lp = cs.light_points(case)
    sid, vlp = cs.schedule(passes)
    dark = ~sp["e"].any(axis=1)
    ok = _lit_diffuse(sp)
    r = cpu_frames(W, H, cam, sp)
    count = {e: 0 for e in cs.witnesses(*case)}
    for s, k in zip(sid, vlp):
        a = r.render_aov(sid=int(s))
        ids = a["id"].reshape(-1)
        p = a["position"].reshape(-1, 3).astype(np.float64)
        n = a["normal"].reshape(-1, 3).astype(np.float64)
        n = n * -np.sign((n * a["dir"].reshape(-1, 3)).sum(-1))[:, None]          # towards the camera ray's side
        q, qn, rad = (lp[k][f].astype(np.float64) for f in ("hp", "nl", "rad"))
        d = q[None] - p
        length = np.linalg.norm(d, axis=-1)
        d /= length[:, None]
        live = (ids >= 0) & ok[np.maximum(ids, 0)] & rad.any() & ((d * qn).sum(-1) < 0) & ((d * n).sum(-1) > 0)
        x = _crossed(p, d, length - EPS, sp)
        free = live & ~(x & dark[None]).any(-1)
        for e in count:
            count[e] += int((free & x[:, e]).sum())
    return count


@pytest.mark.parametrize("case", [c for c in cs.CASES if cs.witnesses(*c)], ids=cs.case_id)
def test_witness_emitters_shadow_enough_pixels(case, cpu_frames):
    count = witness_pairs(case, cs.NPASS, cpu_frames)
    print(f"{cs.case_id(case)}: {count}")
    assert min(count.values()) >= MIN_TWIN_PIXELS, count


@pytest.mark.parametrize("case", [c for c in cs.PRECOMPILED if cs.witnesses(*c)], ids=cs.case_id)
def test_precompiled_witness_emitters_shadow_enough_pixels(case, cpu_frames):
    count = witness_pairs(case, cs.SHORT, cpu_frames)
    print(f"{cs.case_id(case)}: {count}")
    assert min(count.values()) >= MIN_TWIN_PIXELS, count
