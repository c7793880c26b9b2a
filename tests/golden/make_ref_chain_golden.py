"""Regenerate the reference-produced fixtures of the chain buffers, tests/golden/ref_chain_<case>.npz
and ref_chain_meta.json (run from the repo root, on a machine that has the reference tree, after
`make`):

    python tests/golden/make_ref_chain_golden.py

make_ref_aov_golden.py's pin, carried through mirrors and glass: with the probe emission on every
sphere that ends a chain (refl == DIFF, or an emitter already) and none on mirrors and glass
(chain_common.probe_chain_scene), and with dev_lp zero, one pass of the reference's
RadiancePathTracingKernel follows the eye path through the specular vertices and returns, per
channel, throughput * (fabs(dp) * e[id]) of the first non-specular vertex (device.cu:651-660), or +0
when the path misses or runs out of segments.  Everything stored here comes from
oracle/_ref/libref.so (the reference's own device.cu as host C++, oracle/ref.py), one pass with fresh
counters.  Tables: ref.mt607(15) (glass reflects or refracts as the pass decides), the constant
0.875 (P <= 0.75 < 0.875: every glass vertex with a choice refracts, so BDPT_CHAIN_PASS and
BDPT_CHAIN_TRANSMIT coincide; both jitter randoms are 0.875 too) and all zeros (0 < P: every glass
vertex with a choice reflects; the unjittered ray).

Each ref_chain_<case>.npz holds the probe spheres and the scene's own spheres (raw bytes of
SPHERE_DTYPE), the camera (15 floats), the size, sid, the table's name ("seed15", "const0.875",
"zero"; never the table) and the reference's colours whole.

What the fixtures are for is asserted here per case, on the numpy statement of the definition
(tests/chain_common.py np_chain, which calls nothing of the product) -- after that statement's probe
colours have been found equal to the reference's, bit for bit -- and stored in the meta file:
pixels ending after >= 1 mirror bounce in every case, >= 2 glass vertices in the glass cases,
exhausted or >= 4-bounce chains in hall_of_mirrors, total internal reflection somewhere in the set.
hall_of_mirrors' own camera starts every ray outside its small scene (all misses), so the case
looks into the gap between the two mirror balls from HALL_CAMERA instead.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for _p in (REPO, HERE, os.path.dirname(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import oracle  # noqa: E402
import chain_common as cc  # noqa: E402
from make_golden import read_scene_py  # noqa: E402
from make_ref_golden import RAND_N, SCENES, W20, H19  # noqa: E402

SID = 7
SEED15 = "seed15"
HALL_CAMERA = ((0.02, 0.05, -1.2), (0.0, 0.02, 0.0))       # orig, target
COMPLEX_TURNED = 6                                          # visible spheres of complex made SPEC / REFR


def _turn_visible(sp, cam, W, H):
    """The COMPLEX_TURNED spheres of radius < 1000 that cover most pixels of the unjittered frame
    (ties to the lower index) become SPEC and REFR in turn, black and with c = 0.9."""
    zero = np.zeros((H, W), np.float32)
    o, d = cc.camera_rays(cam, W, H, zero, zero)
    _, ids = cc.closest(sp, o.reshape(-1, 3), d.reshape(-1, 3))
    seen, count = np.unique(ids[ids >= 0], return_counts=True)
    keep = sp["rad"][seen] < 1000
    seen, count = seen[keep], count[keep]
    turned = seen[np.lexsort((seen, -count))][:COMPLEX_TURNED]
    assert len(turned) == COMPLEX_TURNED
    for k, s in enumerate(sorted(int(v) for v in turned)):
        sp["refl"][s] = cc.SPEC if k % 2 == 0 else cc.REFR
        sp["e"][s] = 0
        sp["c"][s] = 0.9
    return sorted(int(v) for v in turned)


def _case(name, scene, W, H, table, camera=None, turn=False, note=""):
    orig, target, sp = read_scene_py(os.path.join(SCENES, scene + ".scn"))
    if camera is not None:
        orig, target = (np.array(v, np.float32) for v in camera)
    cam = oracle.update_camera(orig, target, W, H)
    turned = _turn_visible(sp, cam.view(np.float32).reshape(-1), W, H) if turn else []
    return {"name": name, "scene": scene, "W": W, "H": H, "sid": SID, "table": table, "scene_spheres": sp,
            "spheres": cc.probe_chain_scene(sp), "camera": cam, "turned": turned, "note": note}


def cases():
    out = []
    for table, tag in ((SEED15, "s15"), (cc.CONST, "const")):
        what = "glass as the pass decides" if table == SEED15 else "every glass vertex with a choice refracts"
        out.append(_case(f"mirror_{tag}", "cornell_mirror", W20, H19, table, note=f"two mirror walls, a mirror and a glass ball; {what}"))
        out.append(_case(f"glass_{tag}", "cornell_glass", W20, H19, table, note=f"a glass and a mirror ball; total internal reflection inside the glass; {what}"))
        out.append(_case(f"hall_{tag}", "hall_of_mirrors", W20, H19, table, camera=HALL_CAMERA,
                         note=f"into the gap between two mirror balls: chains of up to 7 bounces, exhausted ones; {what}"))
    out.append(_case("mirror_zero", "cornell_mirror", W20, H19, cc.ZERO,
                     note="all-zero table: unjittered rays, every glass vertex with a choice reflects"))
    out.append(_case("mirror_33x9", "cornell_mirror", 33, 9, SEED15, note="a wide frame"))
    out.append(_case("complex_s15", "complex", W20, H19, SEED15, turn=True,
                     note=f"783 spheres (BVH scene), {COMPLEX_TURNED} visible ones turned SPEC / REFR"))
    return out


def run_reference(case, lib, rnd):
    """One pass of the reference's path kernel over the probe scene with zero dev_lp -> colours."""
    lp = np.zeros(oracle.LIGHT_POINTS, oracle.LIGHTPATH_DTYPE)
    col, cnt, _ = lib.path_passes(case["spheres"], rnd, case["camera"], case["W"], case["H"], lp, [case["sid"]], [1])
    assert (cnt == 1).all()
    return col


def statement(case, rnd, branch="pass"):
    return cc.np_chain(case["spheres"], case["camera"].view(np.float32).reshape(-1), case["W"], case["H"], rnd,
                       case["sid"], branch)


def fixture_arrays(case, colors):
    raw = lambda a: np.frombuffer(np.ascontiguousarray(a).tobytes(), np.uint8)  # noqa: E731
    return {"spheres": raw(case["spheres"]), "scene_spheres": raw(case["scene_spheres"]),
            "camera": case["camera"].view(np.float32).reshape(-1),
            "size": np.array([case["W"], case["H"]], np.int32), "sid": np.uint32(case["sid"]),
            "table": np.array(case["table"]), "colors": colors}


def check_coverage(case, cov):
    """What the case is for; `cov` is chain_common.coverage of the statement's PASS chain."""
    name = case["name"]
    assert cov["ended_after_bounce"] > 0, f"{name}: no pixel ends after a mirror bounce"
    if case["scene"] in ("cornell_glass", "cornell_mirror"):
        assert cov["two_glass"] > 0, f"{name}: no chain with two glass vertices"
    if case["scene"] == "hall_of_mirrors":
        assert cov["four_bounces_or_exhausted"] > 0, f"{name}: no long chain"


def main():
    from oracle import ref as R
    lib = R.ref()
    tables, meta, tir = {}, {"rand_n": RAND_N, "sid": SID, "cases": []}, 0
    for case in cases():
        rnd = cc.table_of(case["table"], tables, lib.mt607)
        col = run_reference(case, lib, rnd)
        chain = statement(case, rnd)
        cc.same(cc.probe_chain_colors(case["spheres"], chain), col, f"{case['name']}: the statement against the reference")
        cov = cc.coverage(chain)
        check_coverage(case, cov)
        tir += cov["tir"]
        path = os.path.join(HERE, f"ref_chain_{case['name']}.npz")
        np.savez_compressed(path, **fixture_arrays(case, col))
        meta["cases"].append({"name": case["name"], "scene": case["scene"], "size": [case["W"], case["H"]],
                              "table": case["table"], "spheres": int(len(case["spheres"])),
                              "turned": case["turned"], "coverage": cov, "note": case["note"]})
        print(f"{case['name']:14s} {os.path.getsize(path):6d} B  {cov}")
    assert tir > 0, "no total internal reflection anywhere in the set"
    meta["tir_total"] = tir
    with open(os.path.join(HERE, "ref_chain_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
