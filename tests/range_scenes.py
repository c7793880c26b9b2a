"""Named scenes far outside the numeric range of every other scene of the suite, shared by
tests/test_range_cpu.py and tests/test_gpu_range.py (not a test module, no fixtures).  Everywhere
else coordinates are 0..300, radii 0.3..20 (walls 1e3..1e5) and emission 1..30; here whole scenes
are scaled by exact powers of two, an emitter shrinks to a pin point, and the emission goes to both
ends of float32.  They reach the exec-masked fallbacks behind the range tests of the path kernels
(csrc/bdpt_kernels.hip rcp_rn, rcp_sqrt_rn, the NEE term's library division), denormal radiance in
the fold, the running mean and the units' atomics, and the black-surface exit near its bound.

scene(name) -> (camera with orig/target set, spheres); the caller runs update_camera for its frame.

  base       the box, L, a glass sphere, a mirror and a diffuse ball, the default camera
  far        base x 2^31: every NEE term has len^2 > 2^60 (the library division)
  vast       base x 2^50: in addition the squared lengths passed to the normalisations are >= 2^126
  near       base x 2^-5
  pin_light  base with the emitter's radius 6e-10 and emission 1.2e21: NEE terms on both sides of
             [2^-60, 2^60], and the light pass normalises vectors of squared length < 2^-96
  bright     base with emission 1.9e35 (the black-surface exit's bound is 1e38)
  dim        base with emission 1e-36: some colour values denormal
  dimmer     base with emission 3e-38: nearly every colour value denormal
  horizon    an open scene on the `d < 1e20` rule: see horizon()
  big_far    big_brute(200) x 2^31: a tree scene (bvh_setup's margins, the BVH kernels)
  big_vast   big_brute(200) x 2^50

What the names promise is asserted by tests/test_range_cpu.py from the oracle's range counters
(oracle.RANGE_NAMES), so a scene cannot silently stop meaning what its name says.
"""
import numpy as np

import adversarial_scenes as A
import gpu_bidirectional_raytracer_amd as g
from adversarial_scenes import REFR, SPEC, WHITE, S, box, camera, light, pack

f32 = np.float32

SMALL = ["base", "far", "vast", "near", "pin_light", "bright", "dim", "dimmer", "horizon"]
TREES = ["big_far", "big_vast"]
NAMES = SMALL + TREES
SCALES = {"far": 31, "vast": 50, "near": -5, "big_far": 31, "big_vast": 50}
EMISSION = {"bright": 1.9e35, "dim": 1e-36, "dimmer": 3e-38}
PIN_RAD, PIN_E = 6e-10, 1.2e21
# the scenes on which bdpt_zero_exit_safe's proof holds (the black front wall makes the rule live);
# pin_light's emitter radius is below 2^-16 of the scene's scale, near's emitter is 1/8 from the
# ceiling (the proof wants a gap of 1 at least), horizon has no black surface
ZERO_EXIT = ["base", "far", "vast", "bright", "dim", "dimmer"]
# the emission of `bright` in the preview cases (denoise, reproject, preview_denoise, noise
# estimate); tests/test_range_cpu.py asserts that the CPU backend's outputs are NaN-free at it
PREVIEW_BRIGHT_E = 1.9e35
EMITTER = 6                                              # L's index in base and its variants


def base_rows(rad=A.L_R, e=A.L_E):
    return box() + [S(rad, A.L_P, e=(e,) * 3 if np.isscalar(e) else e, c=A.BLACK),
                    S(12, (35, 20, 70), c=WHITE, refl=REFR), S(12, (65, 20, 70), c=WHITE, refl=SPEC),
                    S(8, (50, 10, 110))]


def scaled(cam, sp, k):
    """Radii, centres and the camera's orig/target times 2^k, exact in float32."""
    s = f32(2.0) ** f32(k)
    sp = sp.copy()
    sp["rad"] *= s
    sp["p"] *= s
    assert np.isfinite(sp["rad"]).all() and np.isfinite(sp["p"]).all()
    for v in (cam.orig, cam.target):
        v.x, v.y, v.z = (float(f32(c) * s) for c in (v.x, v.y, v.z))
    return cam, sp


# horizon.  The reference starts a closest-hit search at t = 1e20f and keeps d only if d < t
# (device.cu:106-124).  No finite float32 hit distance comes near 1e20: the sphere test squares b and
# rad, so a finite det means b < 2^64 and sqrt(det) < 2^64, t < 2^65 = 3.7e19; past that det is NaN or
# -inf (a miss before the rule is asked) or +inf, and then t = +inf.  So the two sides of the rule that
# a scene can reach are: NEAR, a sphere hit at 7e18..1.2e19 (under 1e20, shown), and DOME, a sphere
# around everything with rad = 2e19, rad^2 = +inf, t = +inf (over, never shown: `inf < 1e20f` in the
# generic loop, key_of(+inf) against the running key key_of(1e20f) in the integer keys, and the
# first-hit kernel's copy).  Scaled by 1/2 the dome's rad^2 is finite and it shows on every pixel
# NEAR leaves.  NEAR's hit normals have squared length 1e38 >= 2^126: the first-hit kernel's
# normalisation takes its fallback there.
H_NEAR, H_DOME, H_LIGHT = 0, 1, 2


def horizon(k=0):
    rows = [S(1e19, (1.0e19, 0.0, -1.35e19)), S(2e19, (0.0, 0.0, 0.0)),
            S(1e18, (-6e18, 5e18, -4e18), e=A.L_E, c=A.BLACK)]
    return scaled(camera(o=(0.0, 0.0, 0.0), t=(0.0, 0.0, -1.0)), pack(rows), k)


def scene(name, emission=None):
    """(camera, spheres) of a named scene; `emission` replaces the emitter's in base's variants."""
    if name == "horizon":
        return horizon()
    if name in TREES:
        return scaled(*A.big_brute(200), SCALES[name])
    if name == "pin_light":
        rows = base_rows(PIN_RAD, PIN_E)
    else:
        rows = base_rows(e=EMISSION.get(name, A.L_E) if emission is None else emission)
    cam, sp = camera(), pack(rows)
    return scaled(cam, sp, SCALES[name]) if name in SCALES else (cam, sp)


PREVIEW_WH = (45, 31)


def preview_outputs(name, device):
    """Every preview call on out-of-range radiance, on `device` throughout: the scene's own frame
    after 2 passes (the noise mark) and after 6, denoise() over both material settings,
    noise_estimate(remark=True) and the mark it leaves, then a capture, the camera key 'a', one pass
    of the new view, reproject() and preview_denoise().  -> {what: array}, in call order."""
    from reproject_common import moved
    W, H = PREVIEW_WH
    cam0, sp = scene(name, emission=PREVIEW_BRIGHT_E if name == "bright" else None)
    g.update_camera(cam0, W, H)
    cam1 = moved(cam0, ("a",), W, H)
    sched = g.PassScheduler()
    out = {}
    with g.Renderer(sp, W, H, cam0, device=device) as r:
        r.light_pass(0)
        sched.light()
        r.path_passes(*sched.next(2))
        r.noise_mark()
        r.path_passes(*sched.next(4))
        out["frame"], out["counter"] = r.read_radiance()
        out["denoise"] = r.denoise()
        out["denoise_all"] = r.denoise(levels=5, materials="all")
        for k, v in r.noise_estimate(remark=True, pixels=True).items():
            out["noise_" + k] = np.asarray(v)
        out["mark"], out["mark_counter"] = r.noise_read_mark()
        r.history_capture()
        r.reset_accum()
        r.set_camera(cam1)
        r.path_passes(*sched.next(1))
        out["frame1"] = r.read_radiance()[0]
        out["reproject"], out["reproject_weight"] = r.reproject(weight=True)
        out["preview"], out["preview_weight"] = r.preview_denoise(weight=True)
        out["preview_all"] = r.preview_denoise(levels=5, materials="all")
    return out
