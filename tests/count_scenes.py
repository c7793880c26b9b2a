"""Seeded scenes of an exact sphere count with emitters at exact indices, and the compile-time rules
of the scene-specialised path kernels restated in Python; shared by tests/test_count_scenes_cpu.py
and tests/test_gpu_sphere_counts.py (not a test module, no fixtures).

scene(n, emitters, seed) -> (camera with orig/target set, spheres), 1 <= n <= 64.  The room is
adversarial_scenes.box(): for n >= 8 all six walls (a closed box; where fewer than six spheres are
left for them after the emitters, the missing walls emit), below that as many as fit, the floor
first.  The camera looks down into the room, and every other sphere -- the small non-emitters,
mostly diffuse with a few mirrors, glass and black ones, and the emitters of radius 4 -- hangs in
the part of the room ABOVE the camera's view (LATTICE below).  So at every frame size and under
every jitter a camera ray's first hit is a coloured diffuse wall, which is what makes the ray
counts of the tiny frames predictable (frame_rays), while the segments from those walls to the
light points on the ceiling and the upper walls cross the band where the emitters and the small
spheres hang.  Rows are built first (non-emitters: walls, then small spheres; emitters) and then
placed: the emitters at the given indices in their order, the non-emitters over the other indices
by a seeded permutation, or with a wall kept for index n - 1 (wall_last=True).  A scene without a
non-emitter has nothing to light, so its first emitter sits at the camera's target instead.

The rules (csrc/bdpt_kernels.hip pf_iters, pf_fits and the path loop's choice of lg;
csrc/bdpt_jit_plan.h bdpt_jit_scene::vac_list) are held to the C++ by
tests/test_count_scenes_cpu.py through tests/native/jit_plan_check.cpp.  classes(n, emitters)
names what a specialised build of such a scene contains; UNIVERSE is every class a scene of 1..64
spheres can have; CASES is a list of (n, emitters) that covers it, irredundantly.
"""
import functools

import numpy as np

import adversarial_scenes as adv
import gpu_bidirectional_raytracer_amd as g
import oracle
from adversarial_scenes import BLACK, BLUE, DIFF, GREEN, GREY, RED, REFR, SPEC, WHITE, S, f32

# ---- the scenes -----------------------------------------------------------------------------

CAM_O, CAM_T = (50.0, 60.0, 165.0), (50.0, 0.0, 90.0)      # 38.7 degrees down: the top row looks 9 below level
EMITTER_RAD = 4.0
WALL_ORDER = (2, 4, 0, 1, 3, 5)                            # of adv.box(): floor, back, left, right, ceiling, front
# The band above the view: the view's upper edge falls from the camera (y = 60 at z = 165) by more
# than 0.14 per unit of z (tan 8 degrees; the corner rays are the shallowest, 9.3 degrees), and a
# sphere of radius 4 stays 1.5 above it.  LATTICE: 6 x 2 x 6 cells over x 8..92, that band up to
# y = 75.5 and z 10..110, one sphere per cell, jittered by at most 0.15 / 0.03 / 0.2 of a cell:
# neighbours are at least 9.8 (x), 8.3 (y) and 10 (z) apart, two emitters' radii or more.
NX, NY, NZ = 6, 2, 6
X0, X1, Z0, Z1, Y1 = 8.0, 92.0, 10.0, 110.0, 75.5
COLOURS = (GREY, RED, GREEN, BLUE, WHITE)


def band_floor(z):
    return CAM_O[1] - 0.14 * (CAM_O[2] - z) + EMITTER_RAD + 1.5


def _slot(ix, iy, iz, u):
    x = X0 + (ix + 0.5 + 0.15 * u[0]) * (X1 - X0) / NX
    z = Z0 + (iz + 0.5 + 0.2 * u[2]) * (Z1 - Z0) / NZ
    lo = band_floor(z)
    y = lo + (iy + 0.5 + 0.03 * u[1]) * (Y1 - lo) / NY
    return (f32(x), f32(y), f32(z))


def _small(k, p):
    """The k-th small non-emitter: five diffuse colours, a mirror, a glass ball, a black one."""
    rad = (1.5, 2.5, 2.0, 3.0)[k % 4]
    if k % 8 == 5:
        return S(rad, p, c=WHITE, refl=SPEC)
    if k % 8 == 6:
        return S(rad, p, c=WHITE, refl=REFR)
    if k % 8 == 7:
        return S(rad, p, c=BLACK)
    return S(rad, p, c=COLOURS[k % 5])


def _emitter(k, p):
    return S(EMITTER_RAD, p, e=(12.0, 9.0 + k % 4, 6.0 + 2 * (k % 3)), c=BLACK)


def scene(n, emitters, seed=0, wall_last=False):
    """(camera, spheres): exactly n spheres, emitters at exactly the indices `emitters`."""
    em = sorted(set(int(e) for e in emitters))
    assert 1 <= n <= 64 and all(0 <= e < n for e in em)
    ne, nv = len(em), n - len(em)
    rng = np.random.default_rng(1000 * n + seed)
    walls = adv.box()
    want = 6 if n >= 8 else min(6, nv)
    vac = [walls[w] for w in WALL_ORDER[:min(want, nv)]]
    lit = [S(1e4, walls[w][1], e=(0.5, 0.5, 0.5), c=BLACK) for w in WALL_ORDER[len(vac):want]]
    nwall_vac, nwall_lit = len(vac), len(lit)
    assert nwall_lit <= ne
    # emitters take cells of the middle of the lattice, the small spheres the others
    cells = [(ix, iy, iz) for iz in range(NZ) for ix in range(NX) for iy in range(NY)]
    mid = [c for c in cells if 1 <= c[0] <= NX - 2 and 1 <= c[2] <= NZ - 2]
    rest = [c for c in cells if c not in mid]
    mid = [mid[q] for q in rng.permutation(len(mid))]
    rest = [rest[q] for q in rng.permutation(len(rest))]
    e_cells = mid[:ne - nwall_lit]
    v_cells = (rest + mid[ne - nwall_lit:])[:nv - nwall_vac]
    for k, c in enumerate(e_cells):
        p = _slot(*c, rng.uniform(-1, 1, 3))
        if nv == 0 and k == 0 and not lit:
            p = tuple(f32(v) for v in CAM_T)
        lit.append(_emitter(k, p))
    for k, c in enumerate(v_cells):
        vac.append(_small(k, _slot(*c, rng.uniform(-1, 1, 3))))
    assert len(vac) == nv and len(lit) == ne
    free = [i for i in range(n) if i not in em]
    order = [int(q) for q in rng.permutation(nv)]
    if wall_last:
        assert nwall_vac and free and free[-1] == n - 1
        order.remove(0)
        order.append(0)                                    # row 0, the first wall, goes to index n - 1
    rows = [None] * n
    for i, row in zip(em, lit):
        rows[i] = row
    for i, q in zip(free, order):
        rows[i] = vac[q]
    return adv.camera(CAM_O, CAM_T), adv.pack(rows)


# the precompiled instances bdpt_path_kernel_t<1..16, *> and the generic one at 17 spheres
PRECOMPILED = [(n, (n - 1,)) for n in range(1, 18)] + [(16, (0, 15))]
TINY_FRAMES = [(1, 1), (2, 1), (4, 1), (8, 1), (8, 2), (8, 4)]
# Rounds of at most 8 rays are the only unrolled ones of a list longer than 32 (lg 3..5), and only
# frames of at most 4 pixels start with them: three more such frames, with other pixel centres
MORE_TINY = [(1, 2), (3, 1), (2, 2)]
FULL_FRAME = (45, 31)
NPASS = 16
# The precompiled kernels' 4 passes are passes 6..9 of the schedule: their light points 4 and 5 lie
# on the ceiling above an emitter (the light pass's directions depend on the table alone), so the
# emitter's shadow from them falls into the view; those of passes 0..3 lie below it
SHORT = (6, 4)                                             # (first pass, passes)


# ---- the rules, restated ----------------------------------------------------------------------

PF_MAX_IT = 8                                              # BDPT_PF_MAX_IT


def pf_iters(nl, lg):
    return (nl + (1 << lg) - 1) >> lg


def pf_fits(nl, lg):
    return (1 << (lg - 1)) < nl and pf_iters(nl, lg) <= PF_MAX_IT


def vac_list(n, n_vac):
    return any((1 << k) <= n_vac and pf_iters(n_vac, k) < pf_iters(n, k) for k in (1, 2, 3))


def round_lg(c, nl):
    """log2 of the lane groups of a shadow round of c <= 64 rays over a list of nl spheres: as many
    groups as the rays allow, lowered while half as many still cover the list; 0 = one ray per lane."""
    lg = 5 if c <= 2 else 4 if c <= 4 else 3 if c <= 8 else 2 if c <= 16 else 1 if c <= 32 else 0
    while lg > 0 and (1 << (lg - 1)) >= nl:
        lg -= 1
    return lg


def frame_rays(width, height, step=0):
    """Rays a wave queues at a vertex where every pixel of a frame of at most 64 pixels is at a lit
    diffuse surface: the first emitter's step has its NEE ray and the VLP ray, every later one its
    NEE ray alone."""
    assert width * height <= 64
    return (2 if step == 0 else 1) * width * height


def mask_of(emitters):
    m = 0
    for e in emitters:
        m |= 1 << e
    return m


def _list_classes(name, nl):
    out = set()
    for lg in range(1, 6):
        if (1 << (lg - 1)) >= nl:
            continue
        it = pf_iters(nl, lg)
        kind = "loop" if it > PF_MAX_IT else "tail" if it << lg > nl else "exact"
        assert (kind != "loop") == pf_fits(nl, lg)
        out.add((name, lg, kind, "wide" if nl > 32 else "narrow"))
    return out


def classes(n, emitters):
    """What a specialised build of scene(n, emitters) contains.  Per list ("all": the n spheres;
    "vac": the n_vac non-emitters, where vac_list holds) and lane-group count 2^lg that the list
    reaches: (list, lg, "exact" | "tail" | "loop", "narrow" | "wide") -- unrolled with an exact
    last iteration, unrolled with a masked tail, or the loop; wide = longer than 32.  For the
    "all" list, whose rounds test the emitter mask (width = of n): ("mask", 32 | 64), the type
    the mask is shifted in; ("emitter@", 0 | 31 | 32 | 63), an emitter at an end of a mask word;
    ("emitter@n-1", width); ("emitters", "one" | "several"), several giving rounds of NEE rays
    alone; ("tail_lit" | "tail_dark", lg, width), a masked tail with and without an emitter
    among its candidates; ("iter_lit" | "iter_dark", lg, width), the same of an unrolled iteration
    that is not masked (each (lg, list) is a body of its own, with its own folded constants).  And ("vac_list", bool), ("n_vac=0",), ("no_emitter",)."""
    em = sorted(set(emitters))
    emis, n_vac = mask_of(em), n - len(em)
    # without an emitter no shadow ray is ever queued (a VLP of zero radiance has none), and
    # without a non-emitter every path ends at its first hit: such a build's rounds never run
    if not em:
        return {("no_emitter",)}
    if n_vac == 0:
        return {("n_vac=0",)}
    out = _list_classes("all", n)
    has_vac = vac_list(n, n_vac)
    out.add(("vac_list", has_vac))
    if has_vac:
        out |= _list_classes("vac", n_vac)
    if n >= 2:
        out.add(("mask", 32 if n <= 32 else 64))
    wide = "wide" if n > 32 else "narrow"
    for e in em:
        if e in (0, 31, 32, 63):
            out.add(("emitter@", e))
        if e == n - 1:
            out.add(("emitter@n-1", wide))
    out.add(("emitters", "one" if len(em) == 1 else "several"))
    for lg in range(1, 6):
        if not pf_fits(n, lg):
            continue
        step, it = 1 << lg, pf_iters(n, lg)
        for i in range(it):
            lit = (emis >> (i * step)) & ((1 << step) - 1) != 0
            if i == it - 1 and it * step > n:
                out.add(("tail_lit" if lit else "tail_dark", lg, wide))
            else:
                out.add(("iter_lit" if lit else "iter_dark", lg, wide))
    return out


def _universe():
    """Every class some scene has: the union over all counts and, per count, the emitter sets that
    fill the top indices (every n_vac) and every subset of the ends of the mask words and of the
    list {0, 31, 32, 63, n - 1, n - 2} -- each class in it is reached by one of these scenes."""
    out = set()
    for n in range(1, 65):
        ends = sorted({e for e in (0, 31, 32, 63, n - 1, n - 2) if 0 <= e < n})
        for n_vac in range(0, n + 1):
            out |= classes(n, range(n_vac, n))
        for bits in range(1 << len(ends)):
            out |= classes(n, [e for k, e in enumerate(ends) if bits >> k & 1])
    return out


UNIVERSE = _universe()
REQUIRED_N = (1, 2, 16, 17, 32, 33, 63, 64)

# Each case with what it alone brings (tests/test_count_scenes_cpu.py checks cover and need):
CASES = [
    (1, (0,)),                 # N = 1; no non-emitter
    (2, (1,)),                 # N = 2: one group count, a full mask
    (5, (0,)),                 # dark masked tails at lg 1 and 2
    (7, (6,)),                 # a lit masked tail at lg 1
    (12, (0, 5, 11)),          # a masked tail of the non-emitters' list at lg 1 (9 of 12)
    (16, (15,)),               # N = 16: the last unrolled lg 1, the last precompiled count
    (17, (16,)),               # N = 17: the first loop at lg 1, a one-sphere tail at lg 2..4
    (20, ()),                  # no emitter
    (20, (3,)),                # dark masked tails at lg 3 and 4
    (24, (3, 23)),             # a masked tail of the non-emitters' list at lg 5 (22 of 24)
    (32, (31,)),               # N = 32: bit 31 of the 32-bit mask, one exact iteration at lg 5
    (33, (0,)),                # N = 33: the 64-bit mask with dark one-sphere tails at lg 3..5
    (49, (48,)),               # every emitter at or above 32; exact non-emitters' lists of 48
    (63, (0, 62)),             # N = 63: masked tails one short of full at every lg
    (64, (8, 32, 33, 63)),     # N = 64: bits 32 and 63, exact lists at lg 3..5
]


def case_id(case):
    n, em = case
    return f"n{n}-" + ("none" if not em else "all" if len(em) == n and n > 1 else "e" + "_".join(map(str, em)))


def witnesses(n, emitters):
    """The emitters whose mask bit only this module's scenes exercise: at index >= 32, at index
    n - 1, and among the candidates of a masked tail of an unrolled round over the whole list."""
    out = set()
    if len(set(emitters)) == n:                            # nothing to light: no segment exists
        return []
    for e in emitters:
        if e >= 32 or e == n - 1:
            out.add(e)
        for lg in range(1, 6):
            if pf_fits(n, lg) and pf_iters(n, lg) << lg > n and e >= (pf_iters(n, lg) - 1) << lg:
                out.add(e)
    return sorted(out)


# ---- what the tests share -------------------------------------------------------------------

def schedule(passes=NPASS):
    """(sid, vlp) of the first `passes` passes after a light pass, or of (first, count) of them."""
    s = g.PassScheduler()
    s.light()
    first, count = passes if isinstance(passes, tuple) else (0, passes)
    sid, vlp = s.next(first + count)
    return sid[first:], vlp[first:]


def load(case, width, height):
    cam, sp = scene(*case)
    g.update_camera(cam, width, height)
    return cam, sp


@functools.lru_cache(maxsize=None)
def table(seed):
    rnd = oracle.mt607(seed)
    rnd.setflags(write=False)
    return rnd


def rand0():
    return table(0)


@functools.lru_cache(maxsize=None)
def light_points(case, current_sample=0, after=None):
    """oracle.light_pass at current_sample (on the table of seed 5 * current_sample), from zeros
    or, as in a context that ran light_pass(after) before, from that pass's points: a light ray
    that ends on a mirror, on glass or on an emitter leaves its entry as it was."""
    start = None if after is None else light_points(case, after)
    lp = oracle.light_pass(scene(*case)[1], table(5 * current_sample), current_sample, lp=start)
    lp.setflags(write=False)
    return lp


@functools.lru_cache(maxsize=None)
def expected(case, width, height, passes=NPASS):
    """(colors, counter, pixels) of the oracle after light_pass(0) and schedule(passes), computed
    once per input and left unchanged."""
    cam, sp = load(case, width, height)
    sid, vlp = schedule(passes)
    out = oracle.path_passes(sp, rand0(), cam, width, height, light_points(case), sid, vlp)
    for a in out:
        a.setflags(write=False)
    return out
