"""Named adversarial scenes, shared by tests/test_adversarial_cpu.py and tests/test_gpu_adversarial.py
(not a test module, no fixtures): hit-distance ties between spheres of identical geometry, touching
and concentric spheres, emitters that share their geometry with a non-emitter or touch a wall, an
emitter wall, negative and zero radii, degenerate cameras, and scenes that sit on the BVH builder's
classification limits (csrc/bdpt_bvh.cpp bdpt_build_bvh).  Everything is built in code from float32
values; the only randomness is a seeded choice of positions and a seeded permutation where stated.

The reference scans the spheres from the last down and keeps a hit only if it is nearer (d < t,
device.cu:106-124), so of two spheres that give a ray the same float distance the HIGHER index wins.
Spheres of identical p and rad give every ray identical distances: "twins".

scene(name) -> (camera with orig/target set, spheres); the caller runs update_camera for its frame.
TWINS[name] lists, for the twin scenes, the groups of indices of identical geometry that the camera
must see; what the tests require of them (the CPU test asserts it, so a scene cannot silently stop
meaning what its name says):
  * the CPU backend's un-jittered `id` plane at 45x31 shows the highest index of every listed group
    on at least MIN_TWIN_PIXELS pixels and no lower index of the group on any pixel;
  * twins_large shows at least MIN_LARGE_GROUPS different groups (a group counts when its highest
    index is on at least one pixel -- its spheres are small -- and no lower index is on any);
  * tangent_chain shows every one of CHAIN's spheres.
"""
import numpy as np

import gpu_bidirectional_raytracer_amd as g

f32 = np.float32
DIFF, SPEC, REFR, LITE = g.DIFF, g.SPEC, g.REFR, g.LITE
GREY, RED, GREEN, BLUE, WHITE, BLACK = ((0.75, 0.75, 0.75), (0.75, 0.25, 0.25), (0.25, 0.75, 0.25),
                                        (0.25, 0.25, 0.75), (0.999, 0.999, 0.999), (0.0, 0.0, 0.0))
DARK = (0.0, 0.0, 0.0)
CAM_O, CAM_T = (50.0, 45.0, 168.0), (50.0, 30.0, 60.0)
L_P, L_R, L_E = (50.0, 70.0, 80.0), 6.0, (12.0, 12.0, 12.0)

MIN_TWIN_PIXELS = 20
MIN_LARGE_GROUPS = 10
ID_W, ID_H = 45, 31                 # the frame of the visibility conditions


def S(rad, p, e=DARK, c=GREY, refl=DIFF):
    return (f32(rad), np.array(p, f32), np.array(e, f32), np.array(c, f32), int(refl))


def box(R=1e4):
    """The six walls of test_gpu_fuzz.random_scene around x 0..100, y 0..80, z 0..170 (the wall
    behind the camera is black), indices 0..5: left, right, floor, ceiling, back, front."""
    return [S(R, (-R, 40, 80), c=RED), S(R, (100 + R, 40, 80), c=BLUE), S(R, (50, -R, 80)),
            S(R, (50, 80 + R, 80)), S(R, (50, 40, -R)), S(R, (50, 40, 170 + R), c=BLACK)]


def light(p=L_P, rad=L_R):
    return S(rad, p, e=L_E, c=BLACK)


def pack(rows):
    sp = np.zeros(len(rows), g.SPHERE_DTYPE)
    for i, r in enumerate(rows):
        sp[i] = r
    return sp


def camera(o=CAM_O, t=CAM_T):
    cam = g.Camera()
    cam.orig.x, cam.orig.y, cam.orig.z = (float(f32(v)) for v in o)
    cam.target.x, cam.target.y, cam.target.z = (float(f32(v)) for v in t)
    return cam


A_P, B_P = (35.0, 20.0, 70.0), (65.0, 20.0, 70.0)        # two places the base camera sees well
UP_O, UP_T = (50.0, 50.0, 125.0), (50.0, 64.0, 80.0)    # a camera that sees L well


def _twin_pairs(m_lo, m_hi):
    """Two pairs of identical geometry, the two materials in both index orders: indices 7,8 and 9,10."""
    return box() + [light(), S(9, A_P, c=RED, refl=m_lo), S(9, A_P, c=WHITE, refl=m_hi),
                    S(9, B_P, c=WHITE, refl=m_hi), S(9, B_P, c=GREEN, refl=m_lo)]


def _grid(n, x=(12.0, 88.0), y=(8.0, 50.0), z=(20.0, 130.0), seed=1):
    """n positions on a jittered lattice of the box (seeded), float32."""
    rng = np.random.default_rng(seed)
    k = int(np.ceil(n ** (1 / 3)))
    cells = [(i, j, l) for i in range(k) for j in range(k) for l in range(k)]
    pick = rng.permutation(len(cells))[:n]
    out = []
    for q in pick:
        i, j, l = cells[q]
        u = rng.uniform(0.2, 0.8, 3)
        out.append((f32(x[0] + (i + u[0]) * (x[1] - x[0]) / k), f32(y[0] + (j + u[1]) * (y[1] - y[0]) / k),
                    f32(z[0] + (l + u[2]) * (z[1] - z[0]) / k)))
    return out


MATS = (DIFF, SPEC, REFR, DIFF)
COLS = (RED, WHITE, WHITE, GREEN)
CHAIN = list(range(7, 14))                               # tangent_chain's seven spheres


def _small(name):
    if name == "twin_diff_spec":
        return camera(), _twin_pairs(DIFF, SPEC)
    if name == "twin_refr_diff":
        return camera(), _twin_pairs(REFR, DIFF)
    if name == "twin_emitter_low":                       # the emitter below its diffuse twin
        return camera(UP_O, UP_T), box() + [light(), S(L_R, L_P, c=GREEN), S(9, A_P, c=RED)]
    if name == "twin_emitter_high":
        return camera(UP_O, UP_T), box() + [S(L_R, L_P, c=GREEN), light(), S(9, A_P, c=RED)]
    if name == "twin_black_emitter":                     # a black twin under L, a black mirror elsewhere
        return camera(UP_O, UP_T), box() + [S(L_R, L_P, c=BLACK), light(), S(8, (30, 50, 60), c=BLACK, refl=SPEC)]
    if name == "concentric_glass":
        c = (50.0, 25.0, 70.0)
        return camera(), box() + [light(), S(14, c, c=WHITE, refl=REFR), S(7, c, c=RED),
                                  S(np.nextafter(f32(14), f32(np.inf)), c, c=WHITE, refl=SPEC)]
    if name == "tangent_chain":                          # each touches its neighbours; x = 50 touches the floor
        return camera(), box() + [light()] + [S(5, (20 + 10 * k, 5, 80), c=COLS[k % 4], refl=MATS[k % 3])
                                              for k in range(7)]
    if name == "light_touching_ceiling":                 # tangent to the ceiling wall at (50, 80, 80)
        return camera(UP_O, UP_T), box() + [light(p=(50, 74, 80)), S(8, (40, 50, 70), c=BLACK)]
    if name == "wall_emitter":
        rows = box()
        rows[4] = S(1e4, (50, 40, -1e4), e=L_E, c=BLACK)
        return camera(), rows + [S(10, (50, 20, 70), c=WHITE, refl=REFR)]
    if name == "neg_radius":
        return camera(), box() + [light(), S(-9, A_P, c=RED), S(-8, B_P, c=WHITE, refl=REFR)]
    if name == "neg_radius_emitter":
        return camera(UP_O, UP_T), box() + [light(rad=-6.0), S(9, A_P, c=RED)]
    if name == "zero_radius":
        return camera(), box() + [light(), S(0, (50, 44, 160), c=RED), S(9, A_P, c=GREEN)]
    if name == "tiny_and_huge":                          # 0.6 down the camera axis, half a unit apart
        return camera(), box(1e5) + [light(), S(0.02, (50, 44.9175, 167.4057), c=RED),
                                     S(0.011, (50.5, 44.9175, 167.4057), c=GREEN), S(30, (50, 30, 60), c=WHITE, refl=REFR)]
    if name == "camera_on_surface":                      # |orig - p| == rad exactly
        return camera(), box() + [light(), S(10, (50, 45, 158), c=WHITE, refl=REFR), S(9, A_P, c=RED)]
    if name == "camera_inside_emitter":
        return camera(o=L_P, t=(50, 60, 20)), box() + [light(), S(9, A_P, c=RED)]
    if name == "camera_along_up":                        # straight down: the basis of UpdateCamera degenerates
        return camera(t=(50, 0, 168)), box() + [light(), S(9, A_P, c=RED)]
    raise KeyError(name)


SMALL = ["twin_diff_spec", "twin_refr_diff", "twin_emitter_low", "twin_emitter_high", "twin_black_emitter",
         "concentric_glass", "tangent_chain", "light_touching_ceiling", "wall_emitter", "neg_radius",
         "neg_radius_emitter", "zero_radius", "tiny_and_huge", "camera_on_surface", "camera_inside_emitter",
         "camera_along_up"]
LARGE = ["twins_large", "many_big", "min_tree_23", "min_tree_24", "auto_127", "auto_128"]
NAMES = SMALL + LARGE

# groups of identical geometry the camera must see (module docstring)
TWINS = {"twin_diff_spec": [[7, 8], [9, 10]], "twin_refr_diff": [[7, 8], [9, 10]],
         "twin_emitter_low": [[6, 7]], "twin_emitter_high": [[6, 7]], "twin_black_emitter": [[6, 7]]}

# what bdpt_build_bvh must make of the large scenes: (spheres in the tree, spheres in the brute list),
# tree 0 = no tree at all
CLASSES = {"twins_large": (173, 7), "many_big": (60, 40), "min_tree_23": (0, 29), "min_tree_24": (24, 6),
           "auto_127": (127, 6), "auto_128": (128, 6)}


def _twins_large():
    """6 walls; 40 seeded positions x 4 identical copies, materials cycling; nine identical spheres
    at one point (a leaf holds 4); an emitter under its diffuse twin and a diffuse sphere under its
    emitter twin; one radius-0 point.  The indices after the walls are permuted (seeded), so the
    copies of a group are far apart in index and land in different leaf slots.  180 spheres, 173 in
    the tree, 7 in the brute list.  Returns (camera, spheres, groups)."""
    rng = np.random.default_rng(7)
    rows, grp = [], []
    radii = (f32(3.0), f32(4.0), f32(5.5), f32(2.5))
    for k, p in enumerate(_grid(40, x=(15.0, 85.0), y=(6.0, 48.0), z=(25.0, 120.0), seed=7)):
        for q in range(4):
            rows.append(S(radii[k % 4], p, c=COLS[(k + q) % 4], refl=MATS[(k + q) % 3]))
            grp.append(k)
    for q in range(9):
        rows.append(S(6, (50, 12, 100), c=COLS[q % 4], refl=MATS[q % 3]))
        grp.append(40)
    rows += [S(5, (30, 40, 60), e=L_E, c=BLACK), S(5, (30, 40, 60), c=GREEN)]          # emitter, then its twin
    rows += [S(5, (70, 40, 60), c=RED), S(5, (70, 40, 60), e=L_E, c=BLACK)]
    grp += [41, 41, 42, 42]
    rows.append(S(0, (50, 30, 140), c=RED))
    grp.append(43)
    perm = rng.permutation(len(rows))
    rows, grp = [rows[k] for k in perm], [grp[k] for k in perm]
    for gid, emitter_high in ((41, False), (42, True)):                                 # keep the stated order
        i, j = [k for k, v in enumerate(grp) if v == gid]
        if (rows[j][2].any()) != emitter_high:
            rows[i], rows[j] = rows[j], rows[i]
    groups = [[6 + k for k, v in enumerate(grp) if v == gid] for gid in range(43)]
    return camera(), box() + rows, groups


def _many_big():
    """60 ordinary spheres + 40 for the brute list.  The median radius (bdpt_build_bvh: the n/2-th
    of the sorted signed radii) is 0.5, so the limit is 50: the sphere of radius exactly 50 is in
    the tree, the 24 of radius nextafter(50) are not; 10 points (radius 0) and the 6 walls make 40.
    Three of the 24 are emitters (with an ordinary emitter in the tree as well)."""
    over = np.nextafter(f32(50), f32(np.inf))
    rows = box()
    bumps = [(10 + 16 * i, -45, 20 + 25 * j) for j in range(5) for i in range(5)]       # tops at y = 5: floor bumps
    for k, p in enumerate(bumps[:24]):
        rows.append(S(over, p, e=L_E if k in (3, 11, 18) else DARK, c=COLS[k % 4], refl=MATS[k % 3]))
    rows.append(S(50, bumps[24], c=GREEN))                                            # exactly 100 x the median
    rows.append(light())
    for k, p in enumerate(_grid(13, seed=3)):
        rows.append(S((1.5, 2.0, 3.0)[k % 3], p, c=COLS[k % 4], refl=MATS[k % 3]))
    for k, p in enumerate(_grid(45, y=(6.0, 40.0), z=(90.0, 150.0), seed=4)):
        rows.append(S(0.5, p, c=COLS[k % 4], refl=MATS[k % 3]))
    for k, p in enumerate(_grid(10, seed=5)):
        rows.append(S(0, p, c=RED))
    return camera(), rows


def _counted(n_tree):
    """The box, L and n_tree - 1 spheres of radius 3 on a seeded lattice: n_tree ordinary spheres."""
    rows = box() + [light()]
    for k, p in enumerate(_grid(n_tree - 1, seed=n_tree)):
        rows.append(S(3, p, c=COLS[k % 4], refl=MATS[k % 3]))
    return camera(), rows


def scene(name):
    """(camera, spheres) of a named scene."""
    if name == "twins_large":
        cam, rows, _ = _twins_large()
    elif name == "many_big":
        cam, rows = _many_big()
    elif name in ("min_tree_23", "min_tree_24", "auto_127", "auto_128"):
        cam, rows = _counted(int(name.rsplit("_", 1)[1]))
    else:
        cam, rows = _small(name)
    return cam, pack(rows)


def twin_groups(name):
    return _twins_large()[2] if name == "twins_large" else TWINS.get(name, [])


def has_emitter(sp):
    return bool(sp["e"].any())


def big_brute(n, seed=11):
    """The box, L and n - 7 spheres of radius 1.5 on a seeded lattice; every 50th of them is a copy
    of its predecessor (same p and rad, another colour): the scene of the LDS limit's tests."""
    rows = box() + [light()]
    pts = _grid(n - 7, y=(4.0, 60.0), z=(10.0, 150.0), seed=seed)
    for k, p in enumerate(pts):
        rows.append(S(1.5, pts[k - 1] if k % 50 == 49 else p, c=COLS[k % 4], refl=MATS[k % 3]))
    return camera(), pack(rows)


def write_scn(path, cam, sp):
    """The .scn text of ReadScene (display_func.c:112-175); %.9g round-trips a float32."""
    with open(path, "w") as f:
        o, t = cam.orig, cam.target
        f.write("camera %.9g %.9g %.9g  %.9g %.9g %.9g\n" % (o.x, o.y, o.z, t.x, t.y, t.z))
        f.write("size %d\n" % len(sp))
        for s in sp:
            v = [float(s["rad"]), *map(float, s["p"]), *map(float, s["e"]), *map(float, s["c"])]
            f.write("sphere " + " ".join("%.9g" % x for x in v) + " %d\n" % int(s["refl"]))
