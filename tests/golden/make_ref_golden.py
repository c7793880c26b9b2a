"""Regenerate the reference-produced fixtures tests/golden/ref_*.npz and ref_meta.json (run from
the repo root, on a machine that has the reference tree, after `make`):

    python tests/golden/make_ref_golden.py

Unlike render_*.npz (written by the oracle, make_golden.py) every output here comes from
oracle/_ref/libref.so: the reference's own device.cu and MersenneTwister_kernel.cu compiled as
host C++ (oracle/ref.py).  tests/test_ref_parity.py checks on the CPU that regenerating
reproduces the committed bytes; tests/test_gpu_ref_fixtures.py drives the HIP kernels on the
stored inputs and compares with the stored outputs bit for bit, without the library.

Each ref_<case>.npz holds the inputs (spheres as raw bytes of SPHERE_DTYPE, camera as 15 floats,
size, current_sample, sid, vlp, colors0/counter0 where the accumulation continues) and the
outputs: colors, counter and pixels whole, dev_lp as its fnv1a64 digest plus every 16th row (the
pattern mt607.npz uses for the table).

The edge cases come from the reference's index formulas (rand_count = RAND_N = 7,684,096):
  device.cu:173  i  = (current_sample*5 + ind*4 + seed_id) % (rand_count-4)     GetRayKernel
  device.cu:273  i  = (ind*154 + depth*3 + 4 + seed_id) % (rand_count-3)        light tracing
  device.cu:562  kk = (26 + i*25 + seed_id) % (rand_count-5)                    camera jitter
  device.cu:619  j  = (nn*26 + i*25 + depth*5 + seed_id) % (rand_count-5)       path, nn = 1
The light pass runs with seed_id = 0 (smallpt_cpu.c:330) and ind < 4096, so :173 and :273 never
reach their modulus (15 + 4095*4 and 4095*154 + 4 are far below it); only current_sample moves
them, hence the light pass at current_sample = 3 (table seed 15).  :562 and :619 wrap for
sid >= RAND_N - 5 - 26 - 25*i - 5*depth: wrap_sids() places that threshold on pixels inside the
frame, for depth 0 and for later depths of one path (tests/test_ref_parity.py checks the
arithmetic), and adds sid = RAND_N - 1, the largest value rand() % RAND_N can take.

counts40 is no scene file: tests/count_scenes.py scene(40, (31, 32, 39)), 40 spheres with emitters
on both sides of bit 32 of the specialised kernels' emitter mask, so that the oracle the sweep over
sphere counts (tests/test_gpu_sphere_counts.py) compares with is itself held to the reference at
such a count and layout.
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
from make_golden import read_scene_py  # noqa: E402

RAND_N = oracle.RAND_N
SCENES = os.path.join(REPO, "assets", "scenes")
META = json.load(open(os.path.join(HERE, "render_meta.json")))
SCHED_SID, SCHED_VLP = META["sid"], META["vlp"]        # srand(1) schedule of the first 16 passes
LP_STRIDE = 16
RAND_STRIDE = 997
W20, H19 = 20, 19                                      # one column past the 19x19 launch block


def wrap_sids(W, H):
    """sids whose kk / j index (device.cu:562,619) crosses rand_count-5 inside a W x H frame."""
    m = RAND_N - 5
    i0 = (W * H) // 2
    a = m - 26 - 25 * i0            # kk(i0) = 0: pixels < i0 read the table's end, >= i0 its start
    return [a,                      # pixel i0-1: kk = m-25, j wraps at depth 5
            a + 3,                  # pixel i0-1: kk = m-22, j = m-2 reads past m at depth 4, wraps at 5
            a + 13,                 # pixel i0-1: kk = m-12, wraps at depth 3
            a + 25 * (i0 // 2) + 1,  # the threshold on another pixel (i0 - i0//2), off the 25-grid
            RAND_N - 1]             # every pixel wrapped once; 26 + 25*i + sid stays below 2^32


def kk_index(i, sid):
    return (26 + 25 * i + sid) % 2 ** 32 % (RAND_N - 5)


def j_index(i, depth, sid):
    return (26 + 25 * i + 5 * depth + sid) % 2 ** 32 % (RAND_N - 5)


def _scene(name):
    orig, target, sp = read_scene_py(os.path.join(SCENES, name + ".scn"))
    return orig, target, sp


def _count_scene(n, emitters):
    """tests/count_scenes.py scene(n, emitters) as (orig, target, spheres)."""
    import count_scenes
    cam, sp = count_scenes.scene(n, emitters)
    o, t = cam.orig, cam.target
    return (np.array([o.x, o.y, o.z], np.float32), np.array([t.x, t.y, t.z], np.float32),
            sp.astype(oracle.SPHERE_DTYPE))


def _case(name, scene, W, H, sid, vlp, current_sample=0, edit=None, colors0=None, counter0=None, note="",
          spheres=None):
    orig, target, sp = _scene(scene) if spheres is None else spheres
    if edit is not None:
        edit(sp)
    cam = oracle.update_camera(orig, target, W, H)
    return {"name": name, "scene": scene, "W": W, "H": H, "current_sample": current_sample,
            "sid": np.asarray(sid, np.uint32), "vlp": np.asarray(vlp, np.int32), "spheres": sp,
            "camera": cam, "colors0": colors0, "counter0": counter0, "note": note}


def _no_emitter(sp):
    sp["e"] = 0


def _three_emitters(sp):
    """cornell_2luci's two lamps made unequal, and its glass ball a third, coloured emitter."""
    lit = np.flatnonzero(sp["e"].any(axis=1))
    assert len(lit) == 2
    sp["e"][lit[1]] = (4.0, 9.0, 2.0)
    ball = int(np.flatnonzero((sp["rad"] < 1e3) & ~sp["e"].any(axis=1))[0])
    sp["e"][ball] = (1.0, 0.5, 2.0)
    assert int(sp["e"].any(axis=1).sum()) == 3


def _cap_state(W, H):
    """A running mean in progress: counters straddling the 30000 cap (device.cu:607), a fresh
    pixel and a young one, with non-zero, per-channel different colours."""
    n = W * H
    cnt = np.full(n, 29998, np.uint32)
    cnt[1::7] = 29999
    cnt[3] = 0
    cnt[5] = 7
    col = (0.05 + 0.9 * ((np.arange(3 * n, dtype=np.float64) * 0.6180339887) % 1.0)).astype(np.float32)
    return col.reshape(H, W, 3), cnt.reshape(H, W)


def cases():
    out = []
    for scene in ("cornell", "cornell_glass", "caustic"):
        out.append(_case(f"frame_{scene}", scene, W20, H19, SCHED_SID, SCHED_VLP,
                         note="16 passes of the srand(1) schedule at 20x19"))
    out.append(_case("light_cs3", "cornell_2luci", W20, H19, SCHED_SID[:4], SCHED_VLP[:4], current_sample=3,
                     note="light pass at current_sample=3: table seed 15, GetRayKernel offset 15"))
    out.append(_case("wrap_sid", "cornell_glass", W20, H19, wrap_sids(W20, H19), [1, 1, 2, 2, 3],
                     note="kk/j cross rand_count-5 inside the frame; last sid = RAND_N-1"))
    out.append(_case("vlp4095", "cornell", W20, H19, SCHED_SID[:4], [4095, 0, 4095, 4094],
                     note="the last light point"))
    out.append(_case("one_pixel", "cornell", 1, 1, SCHED_SID, SCHED_VLP, note="1x1 frame, inv_width = 14"))
    c0, n0 = _cap_state(7, 5)
    out.append(_case("cap", "simple", 7, 5, SCHED_SID[:4], SCHED_VLP[:4], colors0=c0, counter0=n0,
                     note="accumulation continued from non-zero colors through the 30000 cap"))
    out.append(_case("no_emitter", "cornell", W20, H19, SCHED_SID[:4], SCHED_VLP[:4], edit=_no_emitter,
                     note="no emitter: dev_lp stays zero; the table is that of seed 0 (the reference "
                          "would leave d_Rand uninitialised, smallpt_cpu.c:311-322)"))
    out.append(_case("three_emitters", "cornell_2luci", W20, H19, SCHED_SID[:6], SCHED_VLP[:6],
                     edit=_three_emitters, note="three unequal emitters, one of them the glass ball"))
    out.append(_case("counts40", "count_scenes.scene(40, (31, 32, 39))", W20, H19, SCHED_SID[:6], SCHED_VLP[:6],
                     spheres=_count_scene(40, (31, 32, 39)),
                     note="40 spheres, emitters at indices 31, 32 and 39: both words of the emitter mask"))
    return out


def lp_rows(lp):
    return np.ascontiguousarray(lp).view(np.float32).reshape(-1, 9)


def run_reference(case, lib, rnd=None):
    """The case through the reference library -> the full outputs (rand, lp, colors, counter, pixels)."""
    rnd = lib.mt607(case["current_sample"] * 5) if rnd is None else rnd
    lp = lib.light_pass(case["spheres"], rnd, case["current_sample"], cam=case["camera"],
                        width=case["W"], height=case["H"])
    col, cnt, px = lib.path_passes(case["spheres"], rnd, case["camera"], case["W"], case["H"], lp,
                                   case["sid"], case["vlp"], colors=case["colors0"], counter=case["counter0"])
    return {"rand": rnd, "lp": lp, "colors": col, "counter": cnt, "pixels": px}


def fixture_arrays(case, res):
    """What ref_<case>.npz stores: inputs, whole small outputs, dev_lp as digest + every 16th row."""
    a = {"spheres": np.frombuffer(np.ascontiguousarray(case["spheres"]).tobytes(), np.uint8),
         "camera": case["camera"].view(np.float32).reshape(-1),
         "size": np.array([case["W"], case["H"]], np.int32),
         "current_sample": np.int32(case["current_sample"]),
         "sid": case["sid"], "vlp": case["vlp"],
         "colors": res["colors"], "counter": res["counter"], "pixels": res["pixels"],
         "lp_fnv": np.uint64(oracle.fnv1a64(lp_rows(res["lp"]))),
         "lp_rows": lp_rows(res["lp"])[::LP_STRIDE].copy()}
    if case["colors0"] is not None:
        a["colors0"], a["counter0"] = case["colors0"], case["counter0"]
    return a


def rand_fixture(lib, seed=15):
    """ref_mt607.npz: the reference's table of the seed of a light pass at current_sample = 3."""
    rnd = lib.mt607(seed)
    idx = np.arange(0, RAND_N, RAND_STRIDE)
    return {"seed": np.uint32(seed), "idx": idx, "values": rnd[idx], "fnv": np.uint64(oracle.fnv1a64(rnd))}


def load_case(name):
    """A committed fixture as the dict the GPU tests use (no reference, no library needed)."""
    g = dict(np.load(os.path.join(HERE, f"ref_{name}.npz")))
    g["spheres"] = np.frombuffer(g["spheres"].tobytes(), oracle.SPHERE_DTYPE).copy()
    g["W"], g["H"] = (int(v) for v in g["size"])
    g["current_sample"] = int(g["current_sample"])
    return g


def main():
    from oracle import ref as R
    lib = R.ref()
    np.savez_compressed(os.path.join(HERE, "ref_mt607.npz"), **rand_fixture(lib))
    tables, meta = {}, {"rand_n": RAND_N, "lp_stride": LP_STRIDE, "rand_stride": RAND_STRIDE,
                        "rand_seed": 15, "cases": []}
    for case in cases():
        seed = case["current_sample"] * 5
        if seed not in tables:
            tables[seed] = lib.mt607(seed)
        res = run_reference(case, lib, tables[seed])
        path = os.path.join(HERE, f"ref_{case['name']}.npz")
        np.savez_compressed(path, **fixture_arrays(case, res))
        meta["cases"].append({"name": case["name"], "scene": case["scene"], "size": [case["W"], case["H"]],
                              "current_sample": case["current_sample"], "table_seed": seed,
                              "sid": case["sid"].tolist(), "vlp": case["vlp"].tolist(), "note": case["note"]})
        print(f"{case['name']:16s} {os.path.getsize(path):7d} B  mean {res['colors'].mean():.5f}  "
              f"lp written {int(res['lp']['rad'].any(axis=1).sum())}")
    with open(os.path.join(HERE, "ref_meta.json"), "w") as f:
        json.dump(meta, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
